"""CPU side of the chain-mapping tests (pesto_amd.chainmap): the NumPy definition of chain_map, the seeded oligomers of the sweep, and the
checks that need no GPU - the definition's assignment against brute force over permutations, the decision margin of every sweep system,
the host-side refusals and apply_mapping on arrays. tests/test_chainmap.py compares the library with this definition on the GPU.

The definition follows the module's docstring: SVD fits (the library's is a Jacobi Kabsch: equal within rounding), an exact assignment by
a subset DP that also keeps the SECOND best total, so that every system can prove that no decision of its search is within rounding:
MARGIN_CAP is a condition on the inputs, not a tolerance."""
import itertools

import numpy as np
import pytest

MARGIN_CAP = 1e-9           # the smallest gap, in units of the TM sum, between the best and the second-best assignment at any visited fit


def d0_def(n):
    return max(0.5, 1.24 * np.cbrt(max(n - 15.0, 0.0)) - 1.8)


def walk(rng, L):
    v = rng.normal(size=(L, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return np.cumsum(3.8 * v, 0)


def rotation(rng):
    q = rng.normal(size=4)
    a, b, c, d = q / np.linalg.norm(q)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a - b * b + c * c - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a - b * b - c * c + d * d]])


def fit_def(X, Y):
    """(R, t) of x' = x @ R + t, the least-squares fit of the points X onto Y; the identity itself where they are equal value for value"""
    if np.array_equal(X, Y):
        return np.eye(3), np.zeros(3)
    mx, my = X.mean(0), Y.mean(0)
    U, _, Vt = np.linalg.svd((X - mx).T @ (Y - my))
    D = np.eye(3)
    D[2, 2] = np.sign(np.linalg.det(U @ Vt))
    R = U @ D @ Vt
    return R, my - mx @ R


_LEVELS = {}


def _levels(cols):
    if cols not in _LEVELS:
        masks = np.arange(1 << cols)
        pop = np.array([bin(m).count("1") for m in masks])
        _LEVELS[cols] = [masks[pop == k] for k in range(cols + 1)]
    return _LEVELS[cols]


def assign_def(S):
    """(best total, gap to the second-best total (inf if there is one assignment only), partner of every row of S or -1): the exact
    maximum of the sum of S over one-to-one assignments of min(rows, columns) pairs, by a subset DP that keeps the two best totals"""
    S = np.asarray(S, np.float64)
    swap = S.shape[0] > S.shape[1]
    M = S.T if swap else S
    rows, cols = M.shape
    levels = _levels(cols)
    f1 = np.full(1 << cols, -np.inf)
    f2 = np.full(1 << cols, -np.inf)
    f1[0] = 0.0
    choice = {}
    for k in range(1, rows + 1):
        masks = levels[k]
        cand = np.full((2 * cols, masks.size), -np.inf)
        for c in range(cols):
            has = (masks >> c & 1) == 1
            sub = masks ^ (1 << c)
            cand[c] = np.where(has, f1[sub] + M[k - 1, c], -np.inf)
            cand[cols + c] = np.where(has, f2[sub] + M[k - 1, c], -np.inf)
        choice[k] = dict(zip(masks.tolist(), np.argmax(cand[:cols], 0).tolist()))
        top = -np.sort(-cand, 0)
        f1[masks], f2[masks] = top[0], top[1]
    last = levels[rows]
    both = np.concatenate([f1[last], f2[last]])
    order = np.argsort(-both, kind="stable")
    best, second = both[order[0]], (both[order[1]] if both.size > 1 else -np.inf)
    mask = int(last[order[0] % last.size])
    part = -np.ones(rows, np.int64)
    for k in range(rows, 0, -1):
        c = choice[k][mask]
        part[k - 1] = c
        mask ^= 1 << c
    if swap:
        out = -np.ones(S.shape[0], np.int64)
        out[part] = np.arange(rows)
        part = out
    return float(best), float(best - second) if np.isfinite(second) else np.inf, part


def chains_of(xyz, offsets):
    return [xyz[offsets[c]:offsets[c + 1]].astype(np.float64) for c in range(len(offsets) - 1)]


def pair_sums(Y, X, R, t, d0, scale):
    """[n_r, n_m] pair sums of the reference chains Y [n_r, L, 3] and the model chains X [n_m, L, 3] under x' = x @ R + t"""
    d = np.linalg.norm((X @ R + t)[None] - Y[:, None], axis=-1) * scale
    return np.nan_to_num(1.0 / (1.0 + (d / d0) ** 2), nan=0.0).sum(-1)


def score_def(ref, rg, mod, mg, R, t, d0, scale):
    """(total, mapping [Cr], pair sum under every reference chain, smallest gap) of the assignment under one transform"""
    total, gap = 0.0, np.inf
    mapping = -np.ones(len(ref), np.int64)
    cs = np.zeros(len(ref))
    for g in sorted(set(rg.tolist()) & set(mg.tolist())):
        ra, mb = np.nonzero(rg == g)[0], np.nonzero(mg == g)[0]
        S = pair_sums(np.stack([ref[a] for a in ra]), np.stack([mod[b] for b in mb]), R, t, d0, scale)
        v, gp, part = assign_def(S)
        total += v
        gap = min(gap, gp)
        for i, a in enumerate(ra):
            if part[i] >= 0:
                mapping[a] = mb[part[i]]
                cs[a] = S[i, part[i]]
    return total, mapping, cs, gap


def common(ya, xb):
    return np.isfinite(ya).all(1) & np.isfinite(xb).all(1)


def cm_def(xyz_ref, ro, rg, frame, mo, mg, n_iter=5, scale=10.0, norm_len=None, d0=None):
    """The definition for one frame: {"seeds": {seed: (total, round, mapping, chain sums, R, t)}, "best": seed, "total", "gap", "L_norm",
    "d0", "finite": the finite slots of every reference chain}; "best" is None for a frame without a seed or with an infinite coordinate"""
    rg, mg = np.asarray(rg), np.asarray(mg)
    ref, mod = chains_of(np.asarray(xyz_ref).reshape(-1, 3), ro), chains_of(frame, mo)
    finite = np.array([np.isfinite(c).all(1).sum() for c in ref])
    Ln = float(finite.sum()) if norm_len is None else float(norm_len)
    dz = d0_def(Ln) if d0 is None else float(d0)
    out = {"seeds": {}, "best": None, "total": -1.0, "gap": np.inf, "L_norm": Ln, "d0": dz, "finite": finite}
    if np.isinf(frame).any() or np.isinf(np.asarray(xyz_ref)).any():
        return out
    Cm = len(mod)
    for a in range(len(ref)):
        for b in range(Cm):
            ok = common(ref[a], mod[b]) if rg[a] == mg[b] else None
            if ok is None or ok.sum() < 3:
                continue
            R, t = fit_def(mod[b][ok], ref[a][ok])
            best, prev = None, None
            for it in range(n_iter):
                total, mapping, cs, gap = score_def(ref, rg, mod, mg, R, t, dz, scale)
                out["gap"] = min(out["gap"], gap)
                if best is None or total > best[0]:
                    best = (total, it, mapping, cs, R, t)
                if prev is not None and np.array_equal(mapping, prev):
                    break
                prev = mapping
                X, Y = [], []
                for aa, bb in enumerate(mapping):
                    if bb >= 0:
                        ok = common(ref[aa], mod[bb])
                        X.append(mod[bb][ok])
                        Y.append(ref[aa][ok])
                X, Y = np.concatenate(X), np.concatenate(Y)
                if len(X) < 3:
                    break
                R, t = fit_def(X, Y)
            out["seeds"][a * Cm + b] = best
            if best[0] > out["total"]:
                out["total"], out["best"] = best[0], a * Cm + b
    return out


# ------------------------------------------------------------------ the systems
def make_system(seed, groups, F=1, noise=1.0, n_nan=2):
    """A planted oligomer. groups: [(L_g, n_ref, n_model)]. Every entity is a random walk of 3.8 A steps; its copies carry their own 0.5 A
    noise and their own rigid placement. The reference holds the first n_ref copies of every group, the model n_model copies (the
    reference's and more, or a random choice of the reference's, frame by frame), shuffled within the group frame by frame, the whole moved rigidly and given ``noise``; n_nan model residues of
    every frame and one reference residue are NaN (chains of fewer than 5 slots are spared). Returns a dict: xyz_ref float32 [Nr, 3],
    ro, rg, xyz float32 [F, Nm, 3], mo, mg, planted int64 [F, Cr] (the model chain that holds every reference chain's copy, or -1)."""
    rng = np.random.default_rng(seed)
    spread = 10.0 + 2.0 * max(L for L, _, _ in groups) ** 0.5
    copies, rg, mg = [], [], []
    for g, (L, n_ref, n_mod) in enumerate(groups):
        base = walk(rng, L)
        base -= base.mean(0)
        n = max(n_ref, n_mod)
        copies.append([(base + rng.normal(scale=0.5, size=base.shape)) @ rotation(rng) + rng.normal(scale=spread, size=3) for _ in range(n)])
        rg += [g] * n_ref
        mg += [g] * n_mod
    ref = [copies[g][c] for g, (L, n_ref, _) in enumerate(groups) for c in range(n_ref)]
    ro = np.concatenate([[0], np.cumsum([len(c) for c in ref])]).astype(np.int32)
    xyz_ref = np.concatenate(ref).astype(np.float32)
    long_ref = [a for a in range(len(ref)) if len(ref[a]) >= 5]
    if long_ref:
        a = long_ref[int(rng.integers(len(long_ref)))]
        xyz_ref[ro[a] + int(rng.integers(len(ref[a])))] = np.nan
    sizes = [groups[g][0] for g in mg]
    mo = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    xyz = np.zeros((F, int(mo[-1]), 3), np.float32)
    planted = -np.ones((F, len(ref)), np.int64)
    for f in range(F):
        R0, t0 = rotation(rng), rng.normal(scale=30.0, size=3)
        b, a0 = 0, 0
        for g, (L, n_ref, n_mod) in enumerate(groups):
            # model chain b + j holds copy held[j]: any n_model of the reference's copies where the model has fewer
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
    return {"xyz_ref": xyz_ref, "ro": ro, "rg": np.array(rg, np.int32), "xyz": xyz, "mo": mo, "mg": np.array(mg, np.int32), "planted": planted}


# (name, seed, groups [(L_g, n_ref, n_model)], F, n_iter, noise): the lane word and its second word (63, 64, 65, 129), the largest
# chain, group sizes 1, 2, 3, 7 and the full 12 x 12 mask table, rows and columns swapped (3 against 5 and 5 against 3), three groups of
# different lengths, groups on one side only, F = 1, 2, 65, n_iter = 1 and 5. A system that misses MARGIN_CAP gets another seed.
SWEEP = [
    ("L3-L4", 1, [(3, 2, 2), (4, 3, 3)], 2, 5, 0.05),
    ("L63-64-65", 2, [(63, 2, 2), (64, 3, 3), (65, 1, 1)], 2, 5, 1.0),
    ("L63-64-65-iter1", 2, [(63, 2, 2), (64, 3, 3), (65, 1, 1)], 2, 1, 1.0),
    ("L129x7", 3, [(129, 7, 7)], 1, 5, 2.0),
    ("L4096x2", 4, [(4096, 2, 2)], 1, 5, 1.0),
    ("L16-12x12", 5, [(16, 12, 12)], 1, 5, 1.0),
    ("3v5", 6, [(40, 3, 5), (20, 1, 1)], 2, 5, 1.5),
    ("5v3", 7, [(40, 5, 3), (20, 1, 1)], 2, 5, 1.5),
    ("one-side", 8, [(30, 2, 2), (25, 2, 0), (35, 0, 1)], 1, 5, 1.0),
    ("F65", 9, [(20, 2, 2), (33, 3, 3)], 65, 5, 1.0),
]
SCALE = 1.0

_CACHE = {}


def sweep_system(name):
    """(system, [definition of every frame]) of a sweep case, computed once and shared (read only)"""
    if name not in _CACHE:
        _, seed, groups, F, n_iter, noise = next(c for c in SWEEP if c[0] == name)
        s = make_system(seed, groups, F, noise)
        _CACHE[name] = (s, [cm_def(s["xyz_ref"], s["ro"], s["rg"], s["xyz"][f], s["mo"], s["mg"], n_iter, SCALE) for f in range(F)])
    return _CACHE[name]


def dyadic_system(sizes=(4,), L=12, seed=11):
    """(reference, model, shuffle): a reference with coordinates on a grid of 1/4 A and the model = the reference with its chains permuted
    within groups, moved by a signed axis permutation (a proper rotation) and a dyadic shift: every coordinate of both is exact in
    float32, and the model IS the reference up to chain order and that motion. shuffle[a] = the model chain that is reference chain a."""
    rng = np.random.default_rng(seed)
    ref, rg = [], []
    for g, n in enumerate(sizes):
        for _ in range(n):
            ref.append(np.round(rng.uniform(-30, 30, size=(L + g, 3)) * 4) / 4)
            rg.append(g)
    rg = np.array(rg, np.int32)
    Q = np.array([[0.0, -1.0, 0.0], [0.0, 0.0, 1.0], [-1.0, 0.0, 0.0]])            # det +1
    order = np.concatenate([np.nonzero(rg == g)[0][rng.permutation(n)] for g, n in enumerate(sizes)])      # model chain j is reference chain order[j]
    mod = [ref[a] @ Q + np.array([8.0, -16.5, 4.25]) for a in order]
    off = lambda cs: np.concatenate([[0], np.cumsum([len(c) for c in cs])]).astype(np.int32)
    return ({"xyz": np.concatenate(ref).astype(np.float32), "offsets": off(ref), "group": rg},
            {"xyz": np.concatenate(mod).astype(np.float32)[None], "offsets": off(mod), "group": rg[order]}, np.argsort(order))


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("shape", [(1, 1), (2, 2), (3, 3), (3, 5), (5, 3), (6, 6), (1, 6), (6, 2)])
def test_the_definitions_assignment_against_brute_force(shape):
    rng = np.random.default_rng(sum(shape) * 7 + shape[0])
    for _ in range(5):
        S = rng.uniform(0, 50, size=shape)
        nr, nm = shape
        M = S.T if nr > nm else S
        totals = sorted((sum(M[i, p[i]] for i in range(M.shape[0])), p) for p in itertools.permutations(range(M.shape[1]), M.shape[0]))
        best, gap, part = assign_def(S)
        assert abs(best - totals[-1][0]) < 1e-12
        assert gap == np.inf if len(totals) == 1 else abs(gap - (totals[-1][0] - totals[-2][0])) < 1e-10
        p = totals[-1][1]
        want = -np.ones(nr, np.int64)
        for i, j in enumerate(p):
            want[j if nr > nm else i] = i if nr > nm else j
        assert np.array_equal(part, want)


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: c[0])
def test_every_sweep_system_keeps_the_margin_and_its_planted_shuffle(case):
    s, defs = sweep_system(case[0])
    for f, d in enumerate(defs):
        assert d["best"] is not None and d["gap"] >= MARGIN_CAP, (f, d["gap"])
        assert np.array_equal(d["seeds"][d["best"]][2], s["planted"][f]), (f, d["seeds"][d["best"]][2], s["planted"][f])


def test_the_dyadic_model_is_its_reference():
    ref, mod, shuffle = dyadic_system((2, 3))
    d = cm_def(ref["xyz"], ref["offsets"], ref["group"], mod["xyz"][0], mod["offsets"], mod["group"], 5, 1.0)
    assert np.array_equal(d["seeds"][d["best"]][2], shuffle) and abs(d["total"] / d["L_norm"] - 1.0) < 1e-12


def test_host_side_refusals_need_no_gpu():
    from pesto_amd import chainmap as C
    s = make_system(1, [(8, 2, 2)])
    args = lambda **k: {**dict(xyz_ref=s["xyz_ref"], ref_offsets=s["ro"], ref_group=s["rg"], xyz=s["xyz"], offsets=s["mo"], group=s["mg"]), **k}
    with pytest.raises(ValueError, match="share its slots"):
        C.chain_map(**args(xyz=s["xyz"][:, :15], offsets=np.array([0, 8, 15])))
    with pytest.raises(ValueError, match="ascend"):
        C.chain_map(**args(offsets=np.array([0, 16, 8])))
    with pytest.raises(ValueError, match="n_iter"):
        C.chain_map(**args(), n_iter=0)
    with pytest.raises(ValueError, match="n_iter"):
        C.chain_map(**args(), n_iter=65)
    with pytest.raises(ValueError, match="scale"):
        C.chain_map(**args(), scale=0.0)
    big = make_system(2, [(3, 13, 1)], n_nan=0)
    with pytest.raises(ValueError, match="at most 12 chains"):
        C.chain_map(big["xyz_ref"], big["ro"], big["rg"], big["xyz"], big["mo"], big["mg"])
    with pytest.raises(ValueError, match="3 to 4096 slots"):
        C.chain_map(**args(xyz=s["xyz"][:, :10], offsets=np.array([0, 8, 10]), group=np.array([0, 1])))
    bad = s["xyz_ref"].copy()
    bad[0, 0] = np.inf
    with pytest.raises(ValueError, match="infinite"):
        C.chain_map(**args(xyz_ref=bad))
    assert C.seed_pair(7, 3) == (2, 1)


def test_apply_mapping_on_arrays():
    from pesto_amd.chainmap import apply_mapping
    x = np.arange(2 * 9 * 3, dtype=np.float32).reshape(2, 9, 3)
    off = np.array([0, 3, 6, 9])
    out = apply_mapping(x, off, np.array([[2, 0, -1], [1, -1, 0]]), off)
    assert out.shape == (2, 9, 3) and out.dtype == np.float32
    assert np.array_equal(out[0, :3], x[0, 6:9]) and np.array_equal(out[0, 3:6], x[0, :3]) and np.isnan(out[0, 6:]).all()
    assert np.array_equal(out[1, :3], x[1, 3:6]) and np.isnan(out[1, 3:6]).all() and np.array_equal(out[1, 6:], x[1, :3])
    assert np.array_equal(apply_mapping(x[0], off, np.array([0, 1, 2]), off), x[:1])
    with pytest.raises(ValueError, match="as many slots"):
        apply_mapping(x, np.array([0, 4, 6, 9]), np.array([0, 1, 2]), off)
