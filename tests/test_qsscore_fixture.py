"""CPU side of the QS-score tests (pesto_amd.qsscore): the NumPy definition of qs_score and, by brute force over all mappings, of qs_map;
the seeded assemblies of the sweep; and the checks that need no GPU - the conditions on the sweep's inputs, n_mappings against
itertools, the definition against hand-worked values and the host-side refusals. tests/test_qsscore.py compares the library with this
definition on the GPU.

The definition follows the module's docstring with dense float64 distance matrices. Three conditions on the inputs make the comparison
one of arithmetic and not of decisions (they are conditions, not tolerances; a system that misses one gets another seed):
    DISTANCE_GAP   no inter-chain distance of a sweep system, on either side, lies within 1e-9 A of 5, 12 or the contact threshold: w
                   jumps by 0.0047 at 12 and the counts are integers, so a pair at a threshold would be a decision
    MAPPING_GAP    the best and the second-best qs_global over all mappings of a qs_map system differ by at least 1e-9
    real contacts  n_ref, n_model and n_shared (under the planted mapping) are all positive, so no sweep case passes on empty sums"""
import itertools
import math

import numpy as np
import pytest

from test_chainmap_fixture import rotation, walk

DISTANCE_GAP = 1e-9
MAPPING_GAP = 1e-9
THR = 8.0
SCALE = 1.0


# ------------------------------------------------------------------ the definition
def w_def(d):
    d = np.asarray(d, np.float64)
    with np.errstate(invalid="ignore"):
        return np.where(d <= 5.0, 1.0, np.where(d < 12.0, np.exp(-2.0 * ((d - 5.0) / 4.28) ** 2), 0.0))


def chains_of(xyz, offsets):
    return [np.asarray(xyz, np.float64).reshape(-1, 3)[offsets[c]:offsets[c + 1]] for c in range(len(offsets) - 1)]


def distances(p, q, scale):
    """[len(p), len(q)] distances, NaN where a point is NaN"""
    return np.linalg.norm(p[:, None] - q[None], axis=-1) * scale


def side_def(chains, thr, scale):
    """(W, n, every finite inter-chain distance) of one side: over ALL chain pairs c < c'"""
    W, n, ds = 0.0, 0, []
    for c in range(len(chains)):
        for cp in range(c + 1, len(chains)):
            d = distances(chains[c], chains[cp], scale)
            d = d[np.isfinite(d)]
            W += float(w_def(d[d < 12.0]).sum())
            n += int((d < thr).sum())
            ds.append(d)
    return W, n, (np.concatenate(ds) if ds else np.zeros(0))


def entry_def(ref, mod, a, ap, b, bp, thr, scale):
    """(num, shared, extra, mref, mmdl, n_shared) of reference interface (a, a') under the model chain pair (b, b')"""
    d1, d2 = distances(ref[a], ref[ap], scale), distances(mod[b], mod[bp], scale)
    common = np.isfinite(d1) & np.isfinite(d2)
    d1, d2 = d1[common], d2[common]
    in1, in2 = d1 < 12.0, d2 < 12.0
    both, one = in1 & in2, in1 ^ in2
    wmin = w_def(np.minimum(d1[both], d2[both]))
    return (float((wmin * (1.0 - np.abs(d1[both] - d2[both]) / 12.0)).sum()), float(wmin.sum()),
            float(w_def(np.where(in1[one], d1[one], d2[one])).sum()), float(w_def(d1[in1]).sum()), float(w_def(d2[in2]).sum()),
            int(((d1 < thr) & (d2 < thr)).sum()))


class FrameDef:
    """The definition for one frame: the totals of both sides and a lazily filled table of entries; score(mapping) gives every output."""

    def __init__(self, xyz_ref, ro, frame, mo, thr=THR, scale=SCALE):
        self.ref, self.mod, self.thr, self.scale = chains_of(xyz_ref, ro), chains_of(frame, mo), thr, scale
        self.bad = bool(np.isinf(np.asarray(frame)).any())
        self.Wref, self.n_ref, self.d_ref = side_def(self.ref, thr, scale)
        self.Wmdl, self.n_mdl, self.d_mdl = (0.0, 0, np.zeros(0)) if self.bad else side_def(self.mod, thr, scale)
        self.table = {}

    def entry(self, a, ap, b, bp):
        key = (a, ap, b, bp)
        if key not in self.table:
            self.table[key] = entry_def(self.ref, self.mod, a, ap, b, bp, self.thr, self.scale)
        return self.table[key]

    def score(self, mapping):
        Cr = len(self.ref)
        nan = float("nan")
        iq = np.full((Cr, Cr), nan)
        if self.bad:
            return {"qs_best": nan, "qs_global": nan, "ics": nan, "ics_precision": nan, "ics_recall": nan, "counts": (-1, -1, -1), "interface_qs": iq}
        num = den = mref = mmdl = 0.0
        n_sh = 0
        for a in range(Cr):
            for ap in range(a + 1, Cr):
                if mapping[a] >= 0 and mapping[ap] >= 0:
                    e = self.entry(a, ap, int(mapping[a]), int(mapping[ap]))
                    num, den, mref, mmdl, n_sh = num + e[0], den + (e[1] + e[2]), mref + e[3], mmdl + e[4], n_sh + e[5]
                    iq[a, ap] = iq[ap, a] = e[0] / (e[1] + e[2]) if e[1] + e[2] > 0 else nan
        dg = den + (self.Wref - mref) + (self.Wmdl - mmdl)
        div = lambda p, q: p / q if q > 0 else nan
        return {"qs_best": div(num, den), "qs_global": div(num, dg), "ics": div(2.0 * n_sh, self.n_ref + self.n_mdl),
                "ics_precision": div(n_sh, self.n_mdl), "ics_recall": div(n_sh, self.n_ref), "counts": (self.n_ref, self.n_mdl, n_sh),
                "interface_qs": iq}


def group_lists(rg, mg):
    rg, mg = np.asarray(rg), np.asarray(mg)
    return [(np.nonzero(rg == g)[0], np.nonzero(mg == g)[0]) for g in sorted(set(rg.tolist()) & set(mg.tolist()))]


def n_mappings_def(rg, mg):
    """by counting: the injective placements of the smaller side of every shared group"""
    n = 1
    for ra, mb in group_lists(rg, mg):
        few, many = sorted((len(ra), len(mb)))
        n *= sum(1 for _ in itertools.permutations(range(many), few))
    return n


def mapping_of_index_def(index, rg, mg):
    """the documented enumeration order, written out independently of the module"""
    m = -np.ones(len(rg), np.int64)
    for ra, mb in group_lists(rg, mg):
        few, many = sorted((len(ra), len(mb)))
        radix = math.factorial(many) // math.factorial(many - few)
        digit, index = index % radix, index // radix
        free = list(range(many))
        for k in range(few):
            q, digit = digit % (many - k), digit // (many - k)
            c = free.pop(q)
            if len(ra) <= len(mb):
                m[ra[k]] = mb[c]
            else:
                m[ra[c]] = mb[k]
    return m


def qs_map_def(fd, rg, mg):
    """{"index", "mapping", "gap" (best minus second-best qs_global; inf with one candidate), "n"}: brute force over all mappings;
    index -1 and a mapping of -1 where no mapping has a qs_global"""
    n = n_mappings_def(rg, mg)
    cands = []
    if not fd.bad:
        for idx in range(n):
            m = mapping_of_index_def(idx, rg, mg)
            s = fd.score(m)
            if s["qs_global"] == s["qs_global"]:
                cands.append((s["qs_global"], s["qs_best"] if s["qs_best"] == s["qs_best"] else -1.0, -idx, m))
    if not cands:
        return {"index": -1, "mapping": -np.ones(len(rg), np.int64), "gap": np.inf, "n": n}
    cands.sort(key=lambda c: c[:3], reverse=True)
    return {"index": -cands[0][2], "mapping": cands[0][3], "gap": cands[0][0] - cands[1][0] if len(cands) > 1 else np.inf, "n": n}


# ------------------------------------------------------------------ the systems
def make_qs_system(seed, groups, F=1, noise=0.3, n_nan=2):
    """A planted assembly whose chains touch. groups: [(L_g, n_ref, n_model)]. Every entity is a random walk of 3.8 A steps; its copies
    carry their own 0.5 A noise and their own rigid placement, their centres a few angstroms apart so that the chains are in contact. The
    reference holds the first n_ref copies of every group; the model n_model copies (the reference's and more, or a random choice of the
    reference's, frame by frame), shuffled within the group frame by frame, the whole moved rigidly and given ``noise``. n_nan random
    residues of every frame and one of the reference are NaN (chains of fewer than 5 slots are spared), and chains of more than 64 slots
    lack slot 63 in the model's first such chain and slot 64 in the reference's last: the edges of the slot block. Returns xyz_ref
    float32 [Nr, 3], ro, rg, xyz float32 [F, Nm, 3], mo, mg, planted int64 [F, Cr]."""
    rng = np.random.default_rng(seed)
    copies, rg, mg = [], [], []
    for g, (L, n_ref, n_mod) in enumerate(groups):
        base = walk(rng, L)
        base -= base.mean(0)
        spread = 2.0 + 0.7 * 3.8 * (L / 6.0) ** 0.5
        copies.append([(base + rng.normal(scale=0.5, size=base.shape)) @ rotation(rng) + rng.normal(scale=spread, size=3) for _ in range(max(n_ref, n_mod))])
        rg += [g] * n_ref
        mg += [g] * n_mod
    ref = [copies[g][c] for g, (L, n_ref, _) in enumerate(groups) for c in range(n_ref)]
    ro = np.concatenate([[0], np.cumsum([len(c) for c in ref])]).astype(np.int32)
    xyz_ref = np.concatenate(ref).astype(np.float32)
    long_ref = [a for a in range(len(ref)) if len(ref[a]) >= 5]
    if long_ref:
        a = long_ref[int(rng.integers(len(long_ref)))]
        xyz_ref[ro[a] + int(rng.integers(len(ref[a])))] = np.nan
    block_ref = [a for a in range(len(ref)) if len(ref[a]) > 64]
    if block_ref:
        xyz_ref[ro[block_ref[-1]] + 64] = np.nan
    sizes = [groups[g][0] for g in mg]
    mo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xyz = np.zeros((F, int(mo[-1]), 3), np.float32)
    planted = -np.ones((F, len(ref)), np.int64)
    for f in range(F):
        R0, t0 = rotation(rng), rng.normal(scale=30.0, size=3)
        b, a0 = 0, 0
        for g, (L, n_ref, n_mod) in enumerate(groups):
            held = rng.permutation(n_ref)[:n_mod] if n_mod < n_ref else rng.permutation(n_mod)
            for j, c in enumerate(held):
                xyz[f, mo[b + j]:mo[b + j + 1]] = (copies[g][c] + rng.normal(scale=noise, size=(L, 3))) @ R0 + t0
                if c < n_ref:
                    planted[f, a0 + c] = b + j
            b += n_mod
            a0 += n_ref
        long_mod = [c for c in range(len(mg)) if sizes[c] >= 5]
        for _ in range(n_nan if long_mod else 0):
            c = long_mod[int(rng.integers(len(long_mod)))]
            xyz[f, mo[c] + int(rng.integers(sizes[c]))] = np.nan
        block_mod = [c for c in range(len(mg)) if sizes[c] > 64]
        if block_mod:
            xyz[f, mo[block_mod[0]] + 63] = np.nan
    return {"xyz_ref": xyz_ref, "ro": ro, "rg": np.array(rg, np.int32), "xyz": xyz, "mo": mo, "mg": np.array(mg, np.int32), "planted": planted}


# (name, seed, groups [(L_g, n_ref, n_model)], F). The table kernel takes 64 slots of the row chain per workgroup (16 per wave) and 64
# slots of the column chain per step: chains of 3, 63, 64, 65 and 129 = two blocks plus one slots; the group make-ups (2), (1, 1),
# (3, 2) and (4); 3 reference chains against 5 model chains and the reverse; a group on one side only; F = 1, 2 and 65 = one above the
# lanes of a wave (the frames of one launch, 32768, are crossed in test_qsscore.py with a tiled system). NaN slots sit at 63 and 64.
SWEEP = [
    ("L3x2", 1, [(3, 2, 2)], 1),
    ("L63-L64", 2, [(63, 1, 1), (64, 1, 1)], 2),
    ("L65x4", 12, [(65, 4, 4)], 1),            # (seed 3 plants the identity: the planted-mapping test wants a shuffle)
    ("L129x3-L40x2", 4, [(129, 3, 3), (40, 2, 2)], 1),
    ("3v5", 5, [(40, 3, 5)], 2),
    ("5v3", 6, [(40, 5, 3)], 2),
    ("one-side", 7, [(30, 2, 2), (25, 2, 0), (35, 0, 1)], 1),
    ("F65", 8, [(20, 2, 2), (33, 1, 1)], 65),
]

_CACHE = {}


def sweep_system(name):
    """(system, [FrameDef of every frame], [qs_map_def of every frame]) of a sweep case, computed once and shared (read only)"""
    if name not in _CACHE:
        _, seed, groups, F = next(c for c in SWEEP if c[0] == name)
        s = make_qs_system(seed, groups, F)
        fds = [FrameDef(s["xyz_ref"], s["ro"], s["xyz"][f], s["mo"]) for f in range(F)]
        _CACHE[name] = (s, fds, [qs_map_def(fd, s["rg"], s["mg"]) for fd in fds])
    return _CACHE[name]


def with_holes(mapping):
    """the mapping with its last mapped entry taken out: a mapping with -1 entries"""
    m = np.array(mapping, np.int64)
    m[np.nonzero(m >= 0)[0][-1]] = -1
    return m


def lattice_system(seed=3, sizes=(2, 1), L=9, box=14.0):
    """A reference on a grid of 1/4 A inside a small box, so that every coordinate is exact in float32 and the chains touch: chains of L,
    L + 1, ... slots by group, one NaN slot. Returns (xyz float32 [N, 3], offsets, group)."""
    rng = np.random.default_rng(seed)
    chains, group = [], []
    for g, n in enumerate(sizes):
        for _ in range(n):
            chains.append(np.round(rng.uniform(0.0, box, size=(L + g, 3)) * 4) / 4)
            group.append(g)
    xyz = np.concatenate(chains).astype(np.float32)
    xyz[4] = np.nan
    return xyz, np.concatenate([[0], np.cumsum([len(c) for c in chains])]).astype(np.int32), np.array(group, np.int32)


def single_pair_system(extra_chain=False):
    """Two chains of three slots with ONE slot pair below 12 A: d1 = 4 in the reference and d2 = 7 in the model; every other pair is far
    away. extra_chain: the model has a third chain of the group whose first slot lies 4 A from the first chain's and sqrt(65) A from the
    second's. Returns (xyz_ref, ro, rg, xyz [1, Nm, 3], mo, mg)."""
    far = [[100.0, 0.0, 0.0], [200.0, 0.0, 0.0]]
    A = np.array([[0.0, 0.0, 0.0]] + far)
    Bfar = [[0.0, 100.0, 0.0], [0.0, 200.0, 0.0]]
    ref = np.concatenate([A, np.array([[4.0, 0.0, 0.0]] + Bfar)]).astype(np.float32)
    mod = [A, np.array([[7.0, 0.0, 0.0]] + Bfar)]
    if extra_chain:
        mod.append(np.array([[0.0, 0.0, -4.0], [0.0, 0.0, -100.0], [0.0, 0.0, -200.0]]))
    n = len(mod)
    return (ref, np.array([0, 3, 6], np.int32), np.zeros(2, np.int32), np.concatenate(mod).astype(np.float32)[None],
            np.arange(n + 1, dtype=np.int32) * 3, np.zeros(n, np.int32))


def threshold_system():
    """single_pair_system with its far slots moved ONTO the thresholds: slot pair (1, 1) lies at exactly 12 A and slot pair (2, 2) at
    exactly 8 A on both sides (integers: exact in float32 and in the distance). 12 is no contact of QS-score (w = 0, the test is <) and 8
    no contact of ICS, but 8 weighs w(8) in the sums."""
    A = np.array([[0.0, 0.0, 0.0], [100.0, 0.0, 0.0], [200.0, 0.0, 0.0]])
    rest = [[112.0, 0.0, 0.0], [208.0, 0.0, 0.0]]
    ref = np.concatenate([A, np.array([[4.0, 0.0, 0.0]] + rest)]).astype(np.float32)
    mod = np.concatenate([A, np.array([[7.0, 0.0, 0.0]] + rest)]).astype(np.float32)
    off = np.array([0, 3, 6], np.int32)
    return ref, off, np.zeros(2, np.int32), mod[None], off, np.zeros(2, np.int32)


def wrong_partner_system(seed=17, LA=60, LB=20):
    """(system, tm mapping, qs mapping): entity A twice (A1, A2, far apart) and entity B once, docked on A1 in the reference. The model
    keeps A1 and A2 where they are (0.2 A of noise) and docks B on A2 in the pose it has on A1 in the reference: every chain is a
    near-rigid copy and two of three superpose, so the TM-like objective of chain_map maps A1 on A1 and A2 on A2; the interface
    (A1, B) of the reference, though, is the model's (A2, B): QS-score maps A1 on A2."""
    rng = np.random.default_rng(seed)
    A = walk(rng, LA)
    A -= A.mean(0)
    B = walk(rng, LB)
    B = B - B.mean(0) + A[LA // 2] + np.array([6.0, 0.0, 0.0])
    R2, t2 = rotation(rng), np.array([120.0, 0.0, 0.0])
    ref = [A, A @ R2 + t2, B]
    mod = [A, A @ R2 + t2, B @ R2 + t2]
    mod = [c + rng.normal(scale=0.2, size=c.shape) for c in mod]
    off = np.array([0, LA, 2 * LA, 2 * LA + LB], np.int32)
    g = np.array([0, 0, 1], np.int32)
    s = {"xyz_ref": np.concatenate(ref).astype(np.float32), "ro": off, "rg": g, "xyz": np.concatenate(mod).astype(np.float32)[None], "mo": off, "mg": g}
    return s, np.array([0, 1, 2]), np.array([1, 0, 2])


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c[0])
def test_every_sweep_system_keeps_its_gaps_and_has_real_contacts(case):
    s, fds, maps = sweep_system(case[0])
    for f, (fd, mp) in enumerate(zip(fds, maps)):
        for d in (fd.d_ref, fd.d_mdl):
            assert d.size and min(np.abs(d - t).min() for t in (5.0, 12.0, THR)) >= DISTANCE_GAP, (f, case[0])
        assert mp["gap"] >= MAPPING_GAP, (f, mp["gap"])
        planted = fd.score(s["planted"][f])
        assert min(planted["counts"]) > 0, (f, planted["counts"])
        holes = fd.score(with_holes(s["planted"][f]))
        assert holes["counts"][0] > 0 and holes["counts"][1] > 0


@pytest.mark.parametrize("name", ["L65x4", "L129x3-L40x2", "3v5"])
def test_the_planted_mapping_has_the_largest_qs_global(name):
    # (not "5v3": a model that holds three of five copies need not hold three that touch, and a chain without a contact scores the same
    # under every reference chain; that case is compared with the brute force only)
    s, fds, maps = sweep_system(name)
    for f, mp in enumerate(maps):
        assert np.array_equal(mp["mapping"], s["planted"][f]), (f, mp["mapping"], s["planted"][f])


def test_the_wrong_partner_system_separates_the_two_objectives():
    s, tm_map, qs_mapping = wrong_partner_system()
    fd = FrameDef(s["xyz_ref"], s["ro"], s["xyz"][0], s["mo"])
    mp = qs_map_def(fd, s["rg"], s["mg"])
    assert np.array_equal(mp["mapping"], qs_mapping) and mp["gap"] >= MAPPING_GAP
    assert fd.score(qs_mapping)["qs_global"] > 0.9 and fd.score(tm_map)["qs_global"] == 0.0
    for d in (fd.d_ref, fd.d_mdl):
        assert min(np.abs(d - t).min() for t in (5.0, 12.0, THR)) >= DISTANCE_GAP


@pytest.mark.parametrize("counts", [((1,), (1,)), ((2,), (2,)), ((3,), (5,)), ((5,), (3,)), ((4, 2), (4, 3)), ((2, 2, 0), (2, 0, 1)), ((6,), (6,))])
def test_n_mappings_against_itertools_and_the_enumeration_is_a_bijection(counts):
    from pesto_amd.qsscore import mapping_of_index, n_mappings
    rg = np.concatenate([[g] * n for g, n in enumerate(counts[0])]).astype(np.int64)
    mg = np.concatenate([[g] * n for g, n in enumerate(counts[1])]).astype(np.int64)[::-1].copy()
    n = n_mappings_def(rg, mg)
    assert n_mappings(rg, mg) == n
    seen = set()
    for idx in range(n):
        m = mapping_of_index(idx, rg, mg)
        assert np.array_equal(m, mapping_of_index_def(idx, rg, mg))
        used = m[m >= 0]
        assert np.unique(used).size == used.size and np.array_equal(rg[m >= 0], mg[used])
        for ra, mb in group_lists(rg, mg):
            assert (m[ra] >= 0).sum() == min(len(ra), len(mb))
        seen.add(tuple(m.tolist()))
    assert len(seen) == n
    with pytest.raises(ValueError, match="index"):
        mapping_of_index(n, rg, mg)


def test_n_mappings_of_the_assemblies_the_limit_is_meant_to_cover():
    from pesto_amd.qsscore import MAX_MAPPINGS, n_mappings
    g = lambda *ns: np.concatenate([[k] * n for k, n in enumerate(ns)])
    assert n_mappings(g(9), g(9)) == math.factorial(9) <= MAX_MAPPINGS
    assert n_mappings(g(6, 6), g(6, 6)) == 720 ** 2 <= MAX_MAPPINGS
    assert n_mappings(g(4, 4, 4), g(4, 4, 4)) == 24 ** 3 <= MAX_MAPPINGS
    assert n_mappings(g(10), g(10)) > MAX_MAPPINGS
    assert n_mappings(g(2), g(0, 3)) == 1


def test_the_definition_against_hand_worked_values():
    assert w_def([0.0, 5.0, 12.0, 11.999999, 20.0]).tolist() == [1.0, 1.0, 0.0, math.exp(-2.0 * ((11.999999 - 5.0) / 4.28) ** 2), 0.0]
    assert abs(float(w_def(12.0 - 1e-12)) - 0.0047) < 1e-4         # the jump at 12
    w7 = math.exp(-2.0 * (2.0 / 4.28) ** 2)
    ref, ro, rg, x, mo, mg = single_pair_system()
    s = FrameDef(ref, ro, x[0], mo).score([0, 1])
    assert s["qs_best"] == 0.75 and s["qs_global"] == 0.75 and s["counts"] == (1, 1, 1) and s["ics"] == 1.0
    assert FrameDef(ref, ro, x[0], mo).entry(0, 1, 0, 1) == (0.75, 1.0, 0.0, 1.0, w7, 1)
    # the chains the other way round: the interface's slot pairs are transposed, (0, 0) stays
    assert FrameDef(ref, ro, x[0], mo).score([1, 0])["qs_best"] == 0.75
    # pairs AT the thresholds: 12 A weighs nothing, 8 A weighs w(8) and is no contact
    w8 = math.exp(-2.0 * (3.0 / 4.28) ** 2)
    ref, ro, rg, x, mo, mg = threshold_system()
    fd = FrameDef(ref, ro, x[0], mo)
    assert fd.entry(0, 1, 0, 1) == (0.75 + w8, 1.0 + w8, 0.0, 1.0 + w8, w7 + w8, 1) and (fd.Wref, fd.n_ref, fd.Wmdl, fd.n_mdl) == (1.0 + w8, 1, w7 + w8, 1)
    assert fd.score([0, 1])["qs_global"] == (0.75 + w8) / (1.0 + w8)
    # a third model chain in contact with both: qs_best stays, qs_global pays for its contacts
    ref, ro, rg, x, mo, mg = single_pair_system(extra_chain=True)
    s = FrameDef(ref, ro, x[0], mo).score([0, 1])
    w65 = math.exp(-2.0 * ((math.sqrt(65.0) - 5.0) / 4.28) ** 2)
    assert s["qs_best"] == 0.75 and abs(s["qs_global"] - 0.75 / (1.0 + 1.0 + w65)) < 1e-15 and s["counts"] == (1, 2, 1)
    assert s["ics_precision"] == 0.5 and s["ics_recall"] == 1.0 and abs(s["ics"] - 2.0 / 3.0) < 1e-15
    # unmapped: nothing shared, every contact counts against the model
    s = FrameDef(ref, ro, x[0], mo).score([0, -1])
    assert s["qs_best"] != s["qs_best"] and s["qs_global"] == 0.0 and s["counts"] == (1, 2, 0) and np.isnan(s["interface_qs"]).all()
    # the lattice reference against itself
    xyz, off, grp = lattice_system()
    s = FrameDef(xyz, off, xyz, off).score([0, 1, 2])
    assert abs(s["qs_best"] - 1.0) < 1e-15 and abs(s["qs_global"] - 1.0) < 1e-15 and s["ics"] == 1.0 and s["counts"][0] > 0


def test_new_names_are_lazy_package_attributes():
    import pesto_amd
    from pesto_amd import qsscore as Q
    for name in ("qsscore", "qs_score", "qs_map", "n_mappings", "mapping_of_index", "interface_points", "structure_qsscore"):
        assert name in pesto_amd.__all__ and getattr(pesto_amd, name) is (Q if name == "qsscore" else getattr(Q, name))


def test_interface_points_stay_inside_their_residue():
    """A glycine followed by a residue WITHOUT a CA (structure_sequences leaves it out) that has a CB, and a chain that ends in a glycine
    with a ligand atom named CB behind it: both glycines keep their CA."""
    from pesto_amd.qsscore import interface_points
    atoms = [("A", 1, "ALA", "N"), ("A", 1, "ALA", "CA"), ("A", 1, "ALA", "C"), ("A", 1, "ALA", "CB"),
             ("A", 2, "GLY", "N"), ("A", 2, "GLY", "CA"), ("A", 2, "GLY", "C"),
             ("A", 3, "SER", "N"), ("A", 3, "SER", "CB"),                                   # no CA: not a listed residue
             ("A", 4, "VAL", "CA"), ("A", 4, "VAL", "CB"),
             ("A", 5, "GLY", "N"), ("A", 5, "GLY", "CA"),
             ("L", 1, "LIG", "CB"), ("L", 1, "LIG", "O1")]
    d = {"xyz": np.arange(len(atoms) * 3, dtype=np.float32).reshape(-1, 3), "chain_name": np.array([a[0] for a in atoms]),
         "resid": np.array([a[1] for a in atoms]), "resname": np.array([a[2] for a in atoms]), "name": np.array([a[3] for a in atoms])}
    pts = interface_points(d)
    assert len(pts) == 1 and pts[0][0] == "A" and pts[0][3].tolist() == [0, 4, 9, 11]
    assert np.array_equal(pts[0][1], d["xyz"][[3, 5, 10, 12]])          # CB of ALA, CA of GLY, CB of VAL, CA of the last GLY


def test_host_side_refusals_need_no_gpu():
    from pesto_amd import qsscore as Q
    s = make_qs_system(1, [(8, 2, 2), (9, 1, 1)])
    args = lambda **k: {**dict(xyz_ref=s["xyz_ref"], ref_offsets=s["ro"], ref_group=s["rg"], xyz=s["xyz"], offsets=s["mo"], group=s["mg"]), **k}
    with pytest.raises(ValueError, match="each at most once"):
        Q.qs_score(**args(), mapping=[0, 0, 2])
    with pytest.raises(ValueError, match="each at most once"):
        Q.qs_score(**args(), mapping=[0, 3, 2])
    with pytest.raises(ValueError, match="one group only"):
        Q.qs_score(**args(), mapping=[0, 2, 1])
    with pytest.raises(ValueError, match=r"mapping must be \[3\] or \[1, 3\]"):
        Q.qs_score(**args(), mapping=[0, 1])
    with pytest.raises(ValueError, match="integers"):
        Q.qs_score(**args(), mapping=[0.0, 1.0, 2.0])
    with pytest.raises(ValueError, match="share its slots"):
        Q.qs_map(**args(xyz=s["xyz"][:, :24], offsets=np.array([0, 8, 15, 24])))
    with pytest.raises(ValueError, match="ascend"):
        Q.qs_map(**args(offsets=np.array([0, 16, 8, 25])))
    with pytest.raises(ValueError, match="3 to 4096 slots"):
        Q.qs_map(**args(xyz=s["xyz"][:, :18], offsets=np.array([0, 8, 16, 18])))
    with pytest.raises(ValueError, match="scale"):
        Q.qs_map(**args(), scale=0.0)
    with pytest.raises(ValueError, match="contact_thr"):
        Q.qs_score(**args(), mapping=[0, 1, 2], contact_thr=float("inf"))
    bad = s["xyz_ref"].copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinite"):
        Q.qs_map(**args(xyz_ref=bad))
    big = make_qs_system(2, [(3, 10, 10)], n_nan=0)
    with pytest.raises(ValueError, match=r"3628800 chain mappings exceed MAX_MAPPINGS = 2\*\*20: find a mapping with chainmap.chain_map"):
        Q.qs_map(big["xyz_ref"], big["ro"], big["rg"], big["xyz"], big["mo"], big["mg"])
    huge = make_qs_system(2, [(3, 13, 1)], n_nan=0)
    with pytest.raises(ValueError, match="at most 12 chains"):
        Q.qs_map(huge["xyz_ref"], huge["ro"], huge["rg"], huge["xyz"], huge["mo"], huge["mg"])
