"""Deterministic case generators of the DSSP sweep (a plain module: tests/test_dssp_sweep_fixture.py checks the generators without a GPU,
tests/test_dssp_sweep.py puts every case through pesto_amd.dssp on one).

The expected outputs come from the loop-level restatement of the definition, ``dssp()`` of tests/golden/make_dssp_golden.py, loaded by
path (tests/golden is no package). A case is a tuple (family, seed, shape); the list below is fixed, so a failure names its case and two
runs execute the same cases. Inputs come from numpy.random.default_rng([seed, attempt]): a builder draws again (attempt 0, 1, ...) until
the definition flags no near-threshold decision (the generator's contract: nothing rests on the last bit of a device sqrt or division)
and the properties the case promises hold. These are properties of the definition alone; no builder looks at the library.

family = kind [+flag ...]; the last entry of every shape is the tuple of promised properties.
    helix   (F, sizes, plan)        backbones from per-residue torsions, placed atom by atom as the generator's ideal() does. The plan names
                                    the segments: x extended (-119 / 113), A alpha (-57 / -47), G 3-10 (-49 / -26), P pi (-57 / -70), 5 a pi
                                    segment of exactly five residues; lengths are seeded, every frame draws its own. A structure of
                                    fewer than 12 residues is all alpha. Plan A500: an alpha helix whose O(1) is moved along C(1) - O(1)
                                    until the last i + 4 -> i bond has e_m = -500 at the middle of its rounding interval (promise em500:
                                    bond() is e_m < -500, so that turn does not start and no H is written). Promises: HI (H directly followed by I), GH, I5 (an isolated run
                                    of exactly five I), Hwins (two consecutive 5-turns whose five residues hold an H: no I is written there)
    sheet   (F, ks, orient, order)  every structure is a sheet of k ideal 8-residue strands, each a chain of its own. A strand is placed from
                                    its parent by a seeded rigid placement (a rotation about the strand axis, a flip for antiparallel, 4.4 ..
                                    5.4 A along the carbonyl direction, +-2 A along the axis) that is kept when the definition codes 12 of
                                    the pair's 16 residues E. orient gives P / A per added strand (cyclically); order 'spatial' places
                                    strand m beside m - 1, 'centre' beside m - 2 (0 in the middle, 1 and 2 on its two sides: a residue of
                                    strand 0 then has bridges to two later strands). Promises: P5 / A5 (a ladder of >= 5 bridges), two (a
                                    residue i with bridges (i, j) of both types), mixed (a residue in a parallel and an antiparallel bridge)
    crop    (F, ((source, n), ..))  windows of n residues of the five recorded structures (the batch of dssp.npz) at seeded offsets, never 0
                                    unless the window is the whole structure. Promises: comp3 (a bulge-linked component of >= 3 ladders),
                                    comp2 (one of exactly 2), oneB (exactly one bridge, coded B at both ends) - all in the first structure
    long    (1, ((source, n), ..))  the windows laid 100 A apart as ONE structure, each with chain numbers of its own
    clash   (F, variant)            a 12-residue alpha helix and a copy displaced by (0.25, 0, 0). No donor N or H comes within 0.5 A of an
                                    acceptor C or O that way (bonded atoms are 1 A apart), so six more copies are planted: three put their
                                    C(2), C(4), C(9) 0.25 A, in seeded directions, from N(6) of the first helix, three their N(3), N(7),
                                    N(10) 0.25 A from its C(5): multi-way ties at the clamp on both sides. Promises: acc9900 / don9900 (a residue whose two best acceptors / donors both have -9900: the
                                    partner index alone orders them). variant 'zero' moves O(4) of the first helix onto C(4) exactly: H(5) is
                                    N + 0 / 0
    bulge   (F, m, orient)          an ideal strand pair as a sheet case places it, with m inert residues inserted behind residue 3 of the
                                    first strand: prolines (no donor) whose four atoms lie within 0.01 A of one point 1.5 A off the sheet
                                    (an acceptor whose C and O coincide has e near 0), so that every C - N step stays below 2.5 A and the
                                    ladder is split on one strand only. Promise: gi4 (two linked ladders with gi = 4, gj <= 1: the far end
                                    of the bulge scan; the recorded structures hold no gi above 2, with noise or without)
flags
    +noise    (crop) every frame is a seeded rigid motion plus Gaussian noise of 0.2 .. 0.3 A, as the golden's frames. Every other case
              with more than one frame moves each frame rigidly and adds 0.02 .. 0.05 A (helix: every frame is a draw of its own besides)
    +nan      one coordinate of one frame is NaN          +pro      about 10 % proline flags
    +missing  about 3 % of the table's entries are -1, among them one of residue 0, of the last residue and of a residue at a structure boundary
    +chains   chain numbers step up at seeded residues, and one C - N bond is stretched by 2 A without a chain change
    +rows     the backbone rows are scattered through n_atoms = 6 R + 3 rows by a seeded permutation; the other rows hold 1e6
    +scale    float32(X / 10) with scale = 10             +far      translated by (9000, -9000, 9000) A before the cast to float32
Edge sets (pesto_dssp.hip): WAVES = 4 subjects per workgroup of the pair pass, its 64-lane walk of a TILE = 128 of partners, NT = 256 threads
of the gather blocks and of the one-workgroup tail (R and R * SLOTS in strides of 256), blockIdx = (frame, block of a structure).
"""
import functools
import importlib.util
import math
import os
import re

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
_spec = importlib.util.spec_from_file_location("make_dssp_golden", os.path.join(GOLDEN, "make_dssp_golden.py"))
G = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(G)                             # (main() is guarded)

H, B, E, NA = 1, 2, 3, 8                              # enum pesto_dssp_code, as the generator's CODES
FAR = np.array([9000.0, -9000.0, 9000.0])
TORSIONS = {"x": (-119.0, 113.0), "A": (-57.0, -47.0), "G": (-49.0, -26.0), "P": (-57.0, -70.0), "5": (-57.0, -70.0)}
LENGTHS = {"A": (7, 11), "G": (5, 9), "P": (6, 10), "5": (5, 6)}            # [low, high) of a helical segment
TRIES = 400

CASES = (
    ("helix", 101, (1, (24,), "xAPx", ("HI", "Hwins"))),
    ("helix", 102, (1, (22,), "xGAx", ("GH",))),
    ("helix", 103, (1, (14,), "x5x", ("I5",))),
    ("helix+pro+scale", 104, (2, (30,), "xAxPx", ())),
    ("helix+nan+rows", 105, (3, (1, 2, 3, 4, 5, 6, 18, 21, 26), "xPAx", ())),
    ("helix+missing+chains", 106, (1, (40, 33), "xAxGxPx", ())),
    ("helix+far", 107, (8, (20,), "xPx", ())),
    ("helix", 108, (2, (4, 5, 6), "A", ())),
    ("helix", 109, (1, (6,), "A500", ("em500",))),
    ("sheet", 201, (1, (2,), "P", "spatial", ("P5",))),
    ("sheet", 202, (1, (2,), "A", "spatial", ("A5",))),
    ("sheet", 203, (1, (3,), "PA", "centre", ("two", "mixed"))),
    ("sheet+rows+pro", 204, (1, (8,), "AP", "spatial", ())),
    ("sheet+scale+far", 205, (2, (4, 3), "PA", "centre", ())),
    ("sheet+chains+missing", 206, (1, (5,), "A", "centre", ())),
    ("sheet+nan", 207, (3, (4,), "PPA", "spatial", ())),
    ("crop", 301, (1, (("1OL5", 65),), ("comp3",))),
    ("crop", 302, (1, (("6O1T", 63),), ("comp2",))),
    ("crop", 303, (1, (("1ZNS", 20),), ("oneB",))),
    ("crop+noise", 304, (2, (("1H9D", 257), ("1ZNS", 1), ("7KHT", 2), ("1OL5", 129), ("6O1T", 3)), ())),
    ("crop+noise", 305, (2, (("1OL5", 63), ("7KHT", 65)), ())),
    ("crop", 306, (1, (("7KHT", 128), ("1H9D", 129)), ())),
    ("crop+rows", 307, (1, (("1OL5", 127),), ())),
    ("crop+scale", 308, (1, (("1H9D", 128),), ())),
    ("crop+far", 309, (1, (("7KHT", 255),), ())),
    ("crop+pro+missing", 310, (1, (("1OL5", 256),), ())),
    ("crop+chains", 311, (1, (("1H9D", 257),), ())),
    ("crop", 312, (1, (("1OL5", 440),), ())),
    ("crop+noise+nan", 313, (3, (("1OL5", 64), ("6O1T", 64), ("1ZNS", 64)), ())),
    ("crop+noise", 314, (8, (("6O1T", 120),), ("comp2",))),
    ("crop+noise", 315, (2, (("1OL5", 70),), ("comp3",))),
    ("long+rows", 401, (1, (("1H9D", 270), ("1OL5", 400), ("6O1T", 400)), ())),
    ("clash", 501, (1, "shift", ("acc9900", "don9900"))),
    ("clash", 502, (1, "zero", ("acc9900", "don9900"))),
    ("clash+nan+rows", 503, (2, "shift", ("acc9900", "don9900"))),
    ("clash+scale+pro", 504, (1, "zero", ("acc9900",))),
    ("clash+far+missing+chains", 505, (1, "shift", ("don9900",))),
    ("bulge", 601, (1, 3, "A", ("gi4",))),
    ("bulge", 602, (2, 3, "P", ("gi4",))),
)


def parse(family):
    kind, *flags = family.split("+")
    return kind, set(flags)


def case_id(case):
    family, seed, shape = case
    flat = []
    for v in shape:
        if isinstance(v, tuple) and v and isinstance(v[0], tuple):
            flat.append("-".join(f"{a}.{b}" for a, b in v))
        elif isinstance(v, tuple):
            flat.append("-".join(str(a) for a in v))
        else:
            flat.append(str(v))
    return f"{family}_s{seed}_" + "x".join(f for f in flat if f)


def every_third(case):
    """the cases that also run from host arrays: every third of a kind"""
    kind = parse(case[0])[0]
    return [c for c in CASES if parse(c[0])[0] == kind].index(case) % 3 == 0


def text(codes):
    return G.text(codes)


def case_sizes(case):
    """(F, residue counts of the case's structures)"""
    kind = parse(case[0])[0]
    shape = case[2]
    if kind == "helix":
        return shape[0], list(shape[1])
    if kind == "sheet":
        return shape[0], [8 * k for k in shape[1]]
    if kind == "crop":
        return shape[0], [n for _, n in shape[1]]
    if kind == "long":
        return shape[0], [sum(n for _, n in shape[1])]
    if kind == "bulge":
        return shape[0], [16 + shape[1]]
    return shape[0], [12 * 8]


# ================================================================== geometry
def backbone(torsions):
    """float64 [4 n, 3]: N, CA, C, O of residues with the given (phi, psi), omega = 180, by the generator's place() as its ideal() does"""
    n = len(torsions)
    Ns, CAs, Cs, Os = [np.array([0.0, 0.0, 0.0])], [np.array([1.458, 0.0, 0.0])], [], []
    Cs.append(np.array([1.458 - 1.525 * math.cos(math.radians(111.0)), 1.525 * math.sin(math.radians(111.0)), 0.0]))
    for i in range(n):
        psi = torsions[i][1]
        Os.append(G.place(Ns[i], CAs[i], Cs[i], 1.231, 120.8, psi + 180.0))
        if i + 1 < n:
            Ns.append(G.place(Ns[i], CAs[i], Cs[i], 1.329, 116.2, psi))
            CAs.append(G.place(CAs[i], Cs[i], Ns[i + 1], 1.458, 121.7, 180.0))
            Cs.append(G.place(Cs[i], Ns[i + 1], CAs[i + 1], 1.525, 111.0, torsions[i + 1][0]))
    return np.stack([np.stack([Ns[i], CAs[i], Cs[i], Os[i]]) for i in range(n)]).reshape(-1, 3)


def rotation(axis, angle):
    a = np.asarray(axis, float) / np.linalg.norm(axis)
    K = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + math.sin(angle) * K + (1.0 - math.cos(angle)) * (K @ K)


def random_rotation(rng):
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


@functools.lru_cache(maxsize=None)
def strand():
    """(the ideal 8-residue strand float64 [32, 3], its centre, its axis, the carbonyl direction across the axis, their normal)"""
    X = backbone([TORSIONS["x"]] * 8)
    ca = X[1::4]
    cen = ca.mean(0)
    ax = np.linalg.svd(ca - cen)[2][0]
    ax = ax if ax @ (ca[-1] - ca[0]) > 0 else -ax
    co = X[3] - X[2]
    u = co - (co @ ax) * ax
    u /= np.linalg.norm(u)
    return X, cen, ax, u, np.cross(ax, u)


@functools.lru_cache(maxsize=None)
def recorded():
    """{name: (X float64 [n_atoms, 3], table, proline, chain)} of the five structures of the golden's batch, each with atom rows of its own"""
    g = np.load(os.path.join(GOLDEN, "dssp.npz"))
    X, table, pro, chain = g["batch_X"][0], g["batch_table"], g["batch_pro"], g["batch_chain"]
    out, r0 = {}, 0
    for name, n in zip(g["batch_names"], g["batch_sizes"].tolist()):
        t = table[r0:r0 + n]
        lo, hi = int(t[t >= 0].min()), int(t.max()) + 1
        out[str(name)[:4]] = (X[lo:hi].astype(np.float64), np.where(t >= 0, t - lo, -1).astype(np.int32), pro[r0:r0 + n].copy(),
                              chain[r0:r0 + n].copy())
        r0 += n
    return out


def window(rng, source, n):
    """a window of n residues of a recorded structure at a seeded offset (never 0 unless it is the whole structure), compacted"""
    X, table, pro, chain = recorded()[source]
    R = table.shape[0]
    o = 0 if n == R else int(rng.integers(1, R - n + 1))
    x, t, p, c = G.compact(X, table, pro, chain, np.arange(o, o + n))
    return x.astype(np.float64), t, p, c, o


def joined(parts):
    """the structures' (X, table, pro, chain) laid end to end: atom rows and chain numbers shifted"""
    atoms = np.cumsum([0] + [p[0].shape[0] for p in parts])
    return (np.concatenate([p[0] for p in parts]), np.concatenate([np.where(p[1] >= 0, p[1] + a, -1) for p, a in zip(parts, atoms)]).astype(np.int32),
            np.concatenate([p[2] for p in parts]).astype(np.uint8), np.concatenate([p[3] for p in parts]).astype(np.int32))


# ================================================================== the definition over a case
def define(X, table, pro, chain, sizes, scale):
    """(codes uint8 [F, R], partners, e_m int32 [F, R, 4], detail [F][structure], the flagged decisions) of the generator's definition"""
    cs, ps, es, details, flagged = [], [], [], [], []
    for f in range(X.shape[0]):
        c1, p1, e1, d1, r0 = [], [], [], [], 0
        for n in sizes:
            d = {}
            c, p, e = G.dssp(X[f], table[r0:r0 + n].tolist(), pro[r0:r0 + n].tolist(), chain[r0:r0 + n].tolist(), scale, flagged, d)
            c1.append(c); p1.append(p); e1.append(e); d1.append(d)
            r0 += n
        cs.append(np.concatenate(c1)); ps.append(np.concatenate(p1)); es.append(np.concatenate(e1)); details.append(d1)
    return np.stack(cs), np.stack(ps), np.stack(es), details, flagged


def structures(c):
    """(frame, structure, codes, partners, e_m, detail) of every (frame, structure) of a built case"""
    for f in range(c["X"].shape[0]):
        r0 = 0
        for s, n in enumerate(c["sizes"]):
            yield f, s, c["codes"][f, r0:r0 + n], c["partners"][f, r0:r0 + n], c["em"][f, r0:r0 + n], c["detail"][f][s]
            r0 += n


def components(detail):
    """{root: number of ladders} of one structure's detail"""
    out = {}
    for r in detail["roots"]:
        out[r] = out.get(r, 0) + 1
    return out


def holds(promise, c):
    """whether a built case has a promised property; read from the definition's outputs alone"""
    for f, s, codes, partners, em, detail in structures(c):
        t = text(codes)
        lad, br = detail["ladders"], detail["bridges"]
        if promise in ("HI", "GH") and promise in t:
            return True
        if promise == "I5" and re.search(r"(?<!I)IIIII(?!I)", t):
            return True
        if promise == "Hwins":
            def bond(d, a):
                return any(partners[d, k] == a and em[d, k] < -500 for k in range(2))
            n = len(codes)
            st = [i + 5 < n and bond(i + 5, i) for i in range(n)]
            if NA not in codes and any(st[i - 1] and st[i] and H in codes[i:i + 5] for i in range(1, n)):
                return True
        if promise == "em500" and any(em[d, k] == -500 and partners[d, k] == d - 4 for d in range(len(codes)) for k in range(2)) and "H" not in t:
            return True
        if promise == "gi4":
            for a, A in enumerate(lad):
                for b, Bl in enumerate(lad):
                    gj = Bl[3] - A[4] - 1 if A[0] == "P" else A[3] - Bl[4] - 1
                    if a != b and A[0] == Bl[0] and detail["roots"][a] == detail["roots"][b] and Bl[1] - A[2] - 1 == 4 and 0 <= gj <= 1:
                        return True
        if promise in ("P5", "A5") and any(L[0] == promise[0] and L[5] >= 5 for L in lad):
            return True
        if promise == "two" and any(len({t2 for (i, _), t2 in br.items() if i == r}) == 2 for r in {i for i, _ in br}):
            return True
        if promise == "mixed" and any(len({t2 for ij, t2 in br.items() if r in ij}) == 2 for r in {r for ij in br for r in ij}):
            return True
        if s == 0:
            comp = components(detail)
            if promise == "comp3" and any(v >= 3 for v in comp.values()):
                return True
            if promise == "comp2" and any(v == 2 for v in comp.values()):
                return True
            if promise == "oneB" and len(br) == 1 and all(codes[r] == B for r in next(iter(br))):
                return True
        if promise == "acc9900" and ((em[:, 0] == -9900) & (em[:, 1] == -9900)).any():
            return True
        if promise == "don9900" and ((em[:, 2] == -9900) & (em[:, 3] == -9900)).any():
            return True
    return False


# ================================================================== the kinds: per-frame float64 coordinates, compact tables
def helix_structure(rng, n, plan):
    if n < 12 or plan == "A":
        return backbone([TORSIONS["A"]] * n)
    for _ in range(50):
        lens = {k: int(rng.integers(*LENGTHS[ch])) for k, ch in enumerate(plan) if ch != "x"}
        nx = [k for k, ch in enumerate(plan) if ch == "x"]
        rest = n - sum(lens.values())
        if rest < 2 * len(nx):
            continue
        cut = np.sort(rng.integers(0, rest - 2 * len(nx) + 1, len(nx) - 1))
        for k, v in zip(nx, np.diff(np.concatenate([[0], cut, [rest - 2 * len(nx)]]))):
            lens[k] = 2 + int(v)
        return backbone([TORSIONS[ch] for k, ch in enumerate(plan) for _ in range(lens[k])])
    return None


def tuned_helix(n):
    """float64 [4 n, 3] of float32 values: the alpha helix whose bond n - 1 -> n - 5 has e_m = -500, by bisection on the position of O(n - 5)"""
    X0 = backbone([TORSIONS["A"]] * n)
    a, d = n - 5, n - 1
    table, zeros = G.plain_table(n).tolist(), [0] * n

    def at(t):
        X = X0.copy()
        X[4 * a + 3] = X0[4 * a + 2] + t * (X0[4 * a + 3] - X0[4 * a + 2])
        X = X.astype(np.float32)
        _, p, e = G.dssp(X, table, zeros, zeros)
        return X, int(e[d][list(p[d, :2]).index(a)]) if a in p[d, :2] else 0

    def first(level):                                   # the smallest t (to 2^-40) with e_m <= level; e_m falls as O moves out
        lo, hi = 0.0, 1.0
        for _ in range(40):
            mid = 0.5 * (lo + hi)
            lo, hi = (lo, mid) if at(mid)[1] <= level else (mid, hi)
        return hi
    X, em = at(0.5 * (first(-500) + first(-501)))
    assert em == -500, em
    return X.astype(np.float64)


def base_helix(rng, shape):
    F, sizes, plan, _ = shape
    if plan == "A500":
        R = sum(sizes)
        return [np.concatenate([tuned_helix(n) for n in sizes])] * F, G.plain_table(R), np.zeros(R, np.uint8), np.zeros(R, np.int32), list(sizes), None
    frames = []
    for _ in range(F):
        xs = [helix_structure(rng, n, plan) for n in sizes]
        if any(x is None for x in xs):
            return None
        frames.append(np.concatenate(xs))
    R = sum(sizes)
    return frames, G.plain_table(R), np.zeros(R, np.uint8), np.zeros(R, np.int32), list(sizes), None


def sheet_structure(rng, k, orient, order):
    """float64 [32 k, 3] or None: the strands in residue order"""
    X0, cen, ax, u, w = strand()
    moves = [(np.eye(3), np.zeros(3))]                  # strand m = (X0 - cen) @ R.T + cen + t
    beside = {0: []}

    def put(m, X):
        R, t = moves[m]
        return (X - cen) @ R.T + cen + t
    for m in range(1, k):
        parent = m - 1 if order == "spatial" or m == 1 else m - 2
        anti = orient[(m - 1) % len(orient)] == "A"
        side = 1.0
        if beside[parent]:                              # away from the neighbour the parent already has, in the parent's own frame
            Rp, tp = moves[parent]
            other = put(beside[parent][0], X0).mean(0)
            side = -1.0 if ((other - cen - tp) @ Rp) @ u > 0 else 1.0
        for _ in range(60):
            R = rotation(ax, math.radians(rng.uniform(-180.0, 180.0)))
            if anti:
                R = rotation(w if rng.random() < 0.5 else u, math.pi) @ R
            t = side * rng.uniform(4.4, 5.4) * u + rng.uniform(-2.0, 2.0) * ax
            pair = np.concatenate([X0, (X0 - cen) @ R.T + cen + t]).astype(np.float32)
            codes = G.dssp(pair, G.plain_table(16).tolist(), [0] * 16, [0] * 8 + [1] * 8)[0]
            if (codes == E).sum() >= 12:
                break
        else:
            return None
        Rp, tp = moves[parent]
        moves.append((Rp @ R, Rp @ t + tp))
        beside[parent].append(m)
        beside[m] = [parent]
    return np.concatenate([put(m, X0) for m in range(k)])


def base_sheet(rng, shape):
    F, ks, orient, order, _ = shape
    xs = [sheet_structure(rng, k, orient, order) for k in ks]
    if any(x is None for x in xs):
        return None
    R = 8 * sum(ks)
    chain = np.concatenate([np.repeat(np.arange(k), 8) for k in ks]).astype(np.int32)
    return [np.concatenate(xs)] * F, G.plain_table(R), np.zeros(R, np.uint8), chain, [8 * k for k in ks], None


def base_crop(rng, shape):
    parts = [window(rng, src, n) for src, n in shape[1]]
    X, table, pro, chain = joined(parts)
    return [X] * shape[0], table, pro, chain, [n for _, n in shape[1]], None


def base_long(rng, shape):
    parts, first = [], 0
    for k, (src, n) in enumerate(shape[1]):
        x, t, p, c, _ = window(rng, src, n)
        x = x - x.mean(0) + np.array([100.0 * k, 0.0, 0.0])
        parts.append((x, t, p, c - c.min() + first))
        first = int(parts[-1][3].max()) + 1
    X, table, pro, chain = joined(parts)
    return [X] * shape[0], table, pro, chain, [table.shape[0]], None


def base_clash(rng, shape):
    F, variant, _ = shape
    X0 = backbone([TORSIONS["A"]] * 12)
    N = lambda r: X0[4 * r]                             # noqa: E731
    C = lambda r: X0[4 * r + 2]                         # noqa: E731
    copies = [X0, X0 + np.array([0.25, 0.0, 0.0])]

    def off():                                          # 0.25 A in a seeded direction
        v = rng.normal(size=3)
        return 0.25 * v / np.linalg.norm(v)
    for a in (2, 4, 9):                                 # C(a) of the copy beside N(6): three acceptors of donor 6 at -9900
        copies.append(X0 + N(6) - C(a) + off())
    for d in (3, 7, 10):                                # N(d) of the copy beside C(5): three donors of acceptor 5 at -9900
        copies.append(X0 + C(5) - N(d) + off())
    R = 12 * len(copies)

    def post(X32, table):
        if variant == "zero":                           # exact: the float32 values themselves are copied
            X32[:, table[4, 3]] = X32[:, table[4, 2]]
    return [np.concatenate(copies)] * F, G.plain_table(R), np.zeros(R, np.uint8), np.repeat(np.arange(len(copies)), 12).astype(np.int32), [R], post


def base_bulge(rng, shape):
    F, m, orient, _ = shape
    X0, cen, ax, u, w = strand()
    pair = sheet_structure(rng, 2, orient, "spatial")
    if pair is None:
        return None
    centre = 0.5 * (X0[4 * 3 + 2] + X0[4 * 4]) + (1.5 if rng.random() < 0.5 else -1.5) * w          # beside the C(3) - N(4) bond
    blobs = centre + rng.uniform(-0.2, 0.2, (m, 1, 3)) + rng.uniform(-0.01, 0.01, (m, 4, 3))
    X = np.concatenate([pair[:16], blobs.reshape(-1, 3), pair[16:]])
    R = 16 + m
    pro = np.zeros(R, np.uint8)
    pro[4:4 + m] = 1
    chain = np.array([0] * (8 + m) + [1] * 8, np.int32)
    return [X] * F, G.plain_table(R), pro, chain, [R], None


BASES = dict(helix=base_helix, sheet=base_sheet, crop=base_crop, long=base_long, clash=base_clash, bulge=base_bulge)


# ================================================================== flags, cast, definition
def draw_case(rng, case):
    family, seed, shape = case
    kind, flags = parse(family)
    base = BASES[kind](rng, shape)
    if base is None:
        return None
    frames, table, pro, chain, sizes, post = base
    frames = [x.copy() for x in frames]
    F, R = len(frames), table.shape[0]
    offs = np.cumsum([0] + sizes)
    full = (table >= 0).all(1)
    stretched = None
    if "chains" in flags:
        marks = np.zeros(R, np.int64)
        marks[rng.integers(0, R, max(1, R // 30))] = 1
        chain = (chain + np.cumsum(marks)).astype(np.int32)
        s = int(np.argmax(sizes))
        x = frames[0]
        ok = [r for r in range(offs[s] + 1, offs[s + 1]) if full[r - 1] and full[r] and chain[r - 1] == chain[r]
              and np.linalg.norm(x[table[r, 0]] - x[table[r - 1, 2]]) <= 2.0]
        if not ok:
            return None
        r = int(ok[int(rng.integers(0, len(ok)))])
        rows = table[r:offs[s + 1]]
        rows = rows[rows >= 0]
        for x in frames:                                # the rest of the structure moves 2 A along C(r - 1) -> N(r)
            v = x[table[r, 0]] - x[table[r - 1, 2]]
            x[rows] += 2.0 * v / np.linalg.norm(v)
        stretched = r
    if F > 1 or "noise" in flags:
        lo, hi = (0.2, 0.3) if "noise" in flags else (0.02, 0.05)
        for f in range(F):
            x = frames[f]
            frames[f] = (x - x.mean(0)) @ random_rotation(rng) + rng.normal(size=3) * 20.0 + rng.normal(size=x.shape) * rng.uniform(lo, hi)
    X = np.stack(frames)
    scale = 1.0
    if "far" in flags:
        X = X + FAR
    if "scale" in flags:
        X, scale = X / 10.0, 10.0
    X = X.astype(np.float32)
    if post is not None:
        post(X, table)
    if "rows" in flags:
        n_atoms = 6 * R + 3
        perm = rng.permutation(n_atoms)[:X.shape[1]]
        wide = np.full((F, n_atoms, 3), 1e6, np.float32)
        wide[:, perm] = X
        X, table = wide, np.where(table >= 0, perm[np.maximum(table, 0)], -1).astype(np.int32)
    if "nan" in flags:
        named = table[table >= 0]
        X[int(rng.integers(0, F)), int(named[int(rng.integers(0, named.size))]), int(rng.integers(0, 3))] = np.nan
    if "missing" in flags:
        table = table.copy()
        must = {0, R - 1, int(offs[1]) - 1 if len(sizes) > 1 else R - 1}
        more = max(0, int(round(0.03 * 4 * R)) - len(must))
        for r in sorted(must | set(rng.integers(0, R, more).tolist())):
            table[r, int(rng.integers(0, 4))] = -1
    if "pro" in flags:
        pro = (pro.astype(bool) | (rng.random(R) < 0.1)).astype(np.uint8)
    codes, partners, em, detail, flagged = define(X, table, pro, chain, sizes, scale)
    if flagged:
        return None
    c = dict(X=X, table=np.ascontiguousarray(table, np.int32), pro=np.ascontiguousarray(pro, np.uint8), chain=np.ascontiguousarray(chain, np.int32),
             sizes=list(sizes), scale=scale, codes=codes, partners=partners, em=em, detail=detail, stretched=stretched)
    if not all(holds(p, c) for p in shape[-1]):
        return None
    return c


def build_fresh(case):
    for attempt in range(TRIES):
        c = draw_case(np.random.default_rng([case[1], attempt]), case)
        if c is not None:
            c["attempt"] = attempt
            return c
    raise AssertionError(f"{case}: no draw in {TRIES} attempts has the promised properties")


@functools.lru_cache(maxsize=None)
def build(case):
    """X float32 [F, n_atoms, 3], table / pro / chain, sizes, scale, and the definition's codes [F, R], partners and em [F, R, 4] in the
    layout of test_dssp_fixture.case, with the detail of every (frame, structure) and the attempt that was kept. Shared: leave it unchanged"""
    return build_fresh(case)


# ================================================================== coverage
def coverage():
    """{name: the set of values the case list hits}"""
    t = {}

    def hit(name, values):
        t.setdefault(name, set()).update(values)
    for case in CASES:
        kind, flags = parse(case[0])
        F, sizes = case_sizes(case)
        hit("sizes", [n if n < 1030 else ">=1030" for n in sizes]); hit("n_struct", [len(sizes)]); hit("F", [F])
        hit("kinds", [kind]); hit("promises", case[2][-1])
        for fl in flags - {"noise"}:
            hit("flag:" + fl, [kind])
        if F >= 2 and len(sizes) >= 2:
            hit("F>=2,n_struct>=2", [case[1]]); hit("F>=2,n_struct>=2:sizes", [tuple(sizes)]); hit("F>=2,n_struct>=2:F*R_total", [F * sum(sizes)])
        hit("F*R_total", [F * sum(sizes)])
        if kind == "crop":                              # the tile and workgroup edges from structures other than 6O1T (never at offset 0)
            hit("edges not from 6O1T", [n for src, n in case[2][1] if src != "6O1T" and n in (127, 128, 129, 255, 256, 257)])
        if F * sum(sizes) > 2000:
            hit("above 2000 residue-frames", [kind])
    return t


# F * R_total = 257 with F >= 2 and two structures does not exist (257 is prime): the 257 case has F = 1 and structures of 128 and 129
REQUIRED = {
    "sizes": {1, 2, 3, 4, 5, 6, 63, 64, 65, 127, 128, 129, 255, 256, 257, 440, ">=1030"}, "n_struct": {1, 2, 3, 9}, "F": {1, 2, 3, 8},
    "kinds": {"helix", "sheet", "crop", "long", "clash", "bulge"},
    "promises": {"HI", "GH", "I5", "Hwins", "P5", "A5", "two", "mixed", "comp3", "comp2", "oneB", "acc9900", "don9900", "em500", "gi4"},
    "F>=2,n_struct>=2:sizes": {(257, 1, 2, 129, 3)}, "F>=2,n_struct>=2:F*R_total": {256}, "F*R_total": {256, 257},
    "edges not from 6O1T": {127, 128, 129, 255, 256, 257},
}
FLAGS = ("nan", "missing", "pro", "chains", "rows", "scale", "far")
