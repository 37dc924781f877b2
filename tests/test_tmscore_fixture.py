"""The NumPy definition of pesto_amd.tmscore (tm_def: float64, the fit by SVD), the hand-worked cases that pin it, the seeded sweep
systems the GPU tests reuse, and the host side of the module. CPU only.

tm_def also returns the per-seed maxima of TM and the DECISION MARGIN: the smallest |d_i - c| over every visited fit and every value
d_i was compared with (each d_cut tried and the five GDT cut-offs). The sweep systems are required to keep that margin >= 1e-7 A: a
condition on the inputs, so that double-precision rounding (about 1e-12 A here) cannot change a set - it is not a tolerance. A case that
falls below gets another seed; the cap is never lowered."""
import functools
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from pesto_amd.tmscore import GDT_CUTOFFS, MAX_RAISE       # the definition's constants, from where a user reads them

CUTS = np.array(GDT_CUTOFFS)
MARGIN_CAP = 1e-7


def seeds_def(L, step=1):
    """[(start, length)]: lengths L >> k (k = 0 .. 5) while above 4, then min(L, 4); starts 0, step, ... <= L - n, plus L - n"""
    lengths, k = [], 0
    while k <= 5 and (L >> k) > 4:
        lengths.append(L >> k)
        k += 1
    lengths.append(min(L, 4))
    out = []
    for n in lengths:
        starts = list(range(0, L - n + 1, step))
        if starts[-1] != L - n:
            starts.append(L - n)
        out += [(s, n) for s in starts]
    return out


def d0_def(norm_len):
    return max(0.5, 1.24 * float(np.cbrt(max(norm_len - 15.0, 0.0))) - 1.8)


def _fits(M, X, Y):
    """the fits of the float64 points X [L, 3] onto Y on the subsets M bool [S, L]: (R [S, 3, 3], m [S, 3], m_ref [S, 3], same [S]), by SVD"""
    ns = M.sum(1, keepdims=True).astype(np.float64)
    Mf = M.astype(np.float64)
    mx, my = Mf @ X / ns, Mf @ Y / ns
    Xc, Yc = X[None] - mx[:, None], Y[None] - my[:, None]
    A = np.einsum("sl,sla,slb->sab", Mf, Xc, Yc)
    U, _, Vt = np.linalg.svd(A)
    d = np.sign(np.linalg.det(U @ Vt))
    D = np.tile(np.eye(3), (M.shape[0], 1, 1))
    D[:, 2, 2] = d
    R = U @ D @ Vt
    same = ~(M & (X != Y).any(1)[None]).any(1)
    R[same] = np.eye(3)
    return R, mx, my, same


def _frame_def(X, Y, seeds, n_iter, scale, d0, lnorm):
    L = X.shape[0]
    S = len(seeds)
    need = min(3, L)
    d_search = min(8.0, max(4.5, d0))
    idx = np.arange(L)
    M = np.array([(idx >= s) & (idx < s + n) for s, n in seeds])
    per_seed = np.full(S, -1.0)
    best_R, best_t = np.zeros((S, 3, 3)), np.zeros((S, 3))
    counts = np.zeros(5, np.int64)
    margin, first_tm = np.inf, None
    active = np.arange(S)
    for _ in range(n_iter):
        if not active.size:
            break
        Ma = M[active]
        R, mx, my, same = _fits(Ma, X, Y)
        P = (X[None] - mx[:, None]) @ R + my[:, None]
        P[same] = X
        D = np.sqrt(((P - Y[None]) ** 2).sum(-1)) * scale
        tm = (1.0 / (1.0 + (D / d0) ** 2)).sum(1) / lnorm
        if first_tm is None:
            first_tm = float(tm[0])
        counts = np.maximum(counts, (D[:, :, None] < CUTS).sum(1).max(0))
        margin = min(margin, float(np.abs(D[:, :, None] - CUTS).min()))
        better = tm > per_seed[active]
        w = active[better]
        per_seed[w] = tm[better]
        best_R[w] = R[better]
        best_t[w] = np.where(same[better, None], 0.0, my[better] - np.einsum("sa,sab->sb", mx[better], R[better]))
        dc = np.full(active.size, d_search)
        raises = np.zeros(active.size, np.int64)
        while True:
            margin = min(margin, float(np.abs(D - dc[:, None]).min()))
            Sn = D < dc[:, None]
            few = (Sn.sum(1) < need) & (raises < MAX_RAISE)
            if not few.any():
                break
            dc[few] += 0.5
            raises[few] += 1
        enough = Sn.sum(1) >= need
        go = enough & (Sn != Ma).any(1)
        M[active[go]] = Sn[go]
        active = active[go]
    return per_seed, best_R, best_t, counts, margin, first_tm


def tm_def(xyz_ref, xyz, sel=None, norm_len=None, d0=None, step=1, n_iter=20, scale=10.0):
    """dict: tm64 float64 [F], tm float32, gdt_ts, gdt_ha float32, counts int32 [F, 5], seed int32, rotation [F, 3, 3], translation [F, 3],
    per_seed float64 [F, n_seeds], margin (the decision margin over all frames), first (TM of the global fit alone) [F]"""
    y = np.asarray(xyz_ref, np.float32).reshape(-1, 3)
    x = np.asarray(xyz, np.float32).reshape(-1, y.shape[0], 3)
    sel = np.arange(y.shape[0]) if sel is None else np.asarray(sel)
    if sel.dtype == bool:
        sel = np.nonzero(sel)[0]
    L, F = sel.size, x.shape[0]
    lnorm = float(L if norm_len is None else norm_len)
    d0 = d0_def(lnorm) if d0 is None else float(d0)
    seeds = seeds_def(L, step)
    Y = y[sel].astype(np.float64)
    out = dict(tm64=np.full(F, np.nan), counts=np.zeros((F, 5), np.int32), seed=np.full(F, -1, np.int32), rotation=np.full((F, 3, 3), np.nan),
               translation=np.full((F, 3), np.nan), per_seed=np.full((F, len(seeds)), np.nan), first=np.full(F, np.nan), margin=np.inf)
    for f in range(F):
        X = x[f, sel].astype(np.float64)
        if not np.isfinite(X).all():
            continue
        per_seed, R, t, counts, margin, first = _frame_def(X, Y, seeds, n_iter, scale, d0, lnorm)
        s = int(np.argmax(per_seed))                    # (the first, so the lowest, seed at the maximum)
        out["tm64"][f], out["seed"][f], out["rotation"][f], out["translation"][f] = per_seed[s], s, R[s], t[s]
        out["counts"][f], out["per_seed"][f], out["first"][f] = counts, per_seed, first
        out["margin"] = min(out["margin"], margin)
    c = out["counts"].astype(np.float64)
    ok = np.isfinite(out["tm64"])
    out["tm"] = out["tm64"].astype(np.float32)
    out["gdt_ts"] = np.where(ok, (c[:, 1] + c[:, 2] + c[:, 3] + c[:, 4]) / (4.0 * L), np.nan).astype(np.float32)
    out["gdt_ha"] = np.where(ok, (c[:, 0] + c[:, 1] + c[:, 2] + c[:, 3]) / (4.0 * L), np.nan).astype(np.float32)
    return out


# ------------------------------------------------------------------ hand-worked cases
def domain16():
    """(ref, model, seed of window (0, 8)): L = 16 on dyadic coordinates in angstroms (scale 1), consecutive atoms more than 8 A apart,
    not collinear; atoms 0..7 of the model are the reference's, atoms 8..15 are shifted by exactly 100 A along x"""
    i = np.arange(16)
    ref = np.stack([16.0 * i, 16.0 * ((i * i) % 5), 16.0 * ((3 * i) % 7)], 1).astype(np.float32)
    assert np.sqrt(((ref[1:] - ref[:-1]) ** 2).sum(1)).min() > 8
    x = ref.copy()
    x[8:, 0] += np.float32(100.0)
    return ref, x[None], seeds_def(16).index((0, 8))


def test_the_seed_windows_by_hand():
    assert CUTS.tolist() == [0.5, 1.0, 2.0, 4.0, 8.0] and MAX_RAISE == 4096
    assert seeds_def(3) == [(0, 3)] and seeds_def(4) == [(0, 4)]
    assert seeds_def(5) == [(0, 5), (0, 4), (1, 4)]
    assert seeds_def(16)[:2] == [(0, 16), (0, 8)] and seeds_def(16)[9:11] == [(8, 8), (0, 4)] and len(seeds_def(16)) == 1 + 9 + 13
    assert seeds_def(11, 4) == [(0, 11), (0, 5), (4, 5), (6, 5), (0, 4), (4, 4), (7, 4)]
    assert [n for s, n in seeds_def(4096, 4096)] == [4096, 2048, 2048, 1024, 1024, 512, 512, 256, 256, 128, 128, 4, 4]
    from pesto_amd import tmscore as T
    for L, step in ((3, 1), (5, 1), (16, 1), (11, 4), (257, 4), (4096, 4096)):
        assert T.seed_windows(L, step).tolist() == [list(w) for w in seeds_def(L, step)]
    assert d0_def(16) == 0.5 and abs(d0_def(300) - (1.24 * 285 ** (1 / 3) - 1.8)) < 1e-12
    assert np.array_equal(T.default_d0([16, 300]), [d0_def(16), d0_def(300)])


def test_a_model_that_is_the_reference():
    ref, _, _ = domain16()
    got = tm_def(ref, ref[None], scale=1.0)
    assert got["tm64"][0] == 1.0 and got["counts"][0].tolist() == [16] * 5 and got["seed"][0] == 0
    assert got["gdt_ts"][0] == 1.0 and got["gdt_ha"][0] == 1.0
    assert np.array_equal(got["rotation"][0], np.eye(3)) and np.array_equal(got["translation"][0], np.zeros(3))


def test_displaced_domain_by_hand():
    ref, x, w = domain16()
    got = tm_def(ref, x, scale=1.0)
    assert d0_def(16) == 0.5 and w == 1
    assert got["tm64"][0] == (8 + 8 / 40001) / 16 and got["counts"][0].tolist() == [8] * 5 and got["seed"][0] == w
    assert got["gdt_ts"][0] == np.float32(0.5) and got["gdt_ha"][0] == np.float32(0.5)
    assert np.array_equal(got["rotation"][0], np.eye(3)) and np.array_equal(got["translation"][0], np.zeros(3))
    assert got["first"][0] < 0.05 < got["tm64"][0]                     # one global superposition sees neither domain in place


def test_single_seed_lengths_and_a_nan_frame():
    for L in (3, 4):
        s = sweep_system(L, 2, 7)
        got = tm_def(s["ref"], s["xyz"])
        assert got["per_seed"].shape == (2, 1) and (got["seed"] == 0).all() and (0 < got["tm64"]).all() and (got["tm64"] < 1).all()
    s = sweep_system(5, 3, 1)
    x = s["xyz"].copy()
    x[1, 2, 1] = np.nan
    got = tm_def(s["ref"], x)
    assert np.isnan(got["tm"][1]) and np.isnan(got["gdt_ts"][1]) and np.isnan(got["gdt_ha"][1]) and got["seed"][1] == -1
    assert (got["counts"][1] == 0).all() and np.isfinite(got["tm"][[0, 2]]).all() and (got["seed"][[0, 2]] >= 0).all()


# ------------------------------------------------------------------ the sweep systems
def _rotation(rng, angle):
    a = rng.normal(size=3)
    a /= np.linalg.norm(a)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


@functools.lru_cache(maxsize=None)
def sweep_system(L, F, seed):
    """dict(ref float32 [L, 3], xyz float32 [F, L, 3]) in nanometres (scale 10): a CA-like trace with steps of 3.8 A; every frame is the
    trace with 1 A of noise and its second half moved as a rigid domain (a rotation of 20 to 60 degrees about the domain's centre and a
    shift of a few angstroms), rounded to float32"""
    rng = np.random.default_rng(1000 * L + seed)
    step = rng.normal(size=(L, 3))
    for k in range(1, L):
        step[k] += 0.8 * step[k - 1]                     # a persistent walk: compact, not a line
        step[k] /= np.linalg.norm(step[k])
    step[0] /= np.linalg.norm(step[0])
    ref = np.cumsum(3.8 * step, 0)
    xyz = np.empty((F, L, 3))
    h = L // 2
    for f in range(F):
        m = ref + rng.normal(size=(L, 3))
        c = m[h:].mean(0)
        m[h:] = (m[h:] - c) @ _rotation(rng, np.deg2rad(rng.uniform(20, 60))) + c + rng.normal(size=3) * 3.0
        xyz[f] = m
    return dict(ref=(0.1 * ref).astype(np.float32), xyz=(0.1 * xyz).astype(np.float32))


# (L, F, step, seed of the system; seed 0 of (64, 65) fell below the margin cap, at 1.4e-8 A): the lane word and its second word (63, 64, 65, 129, 257), the single-seed lengths, F of 1, 2, 65
SWEEP = [(3, 2, 1, 0), (4, 65, 1, 0), (5, 65, 1, 0), (63, 2, 1, 0), (64, 65, 1, 2), (65, 1, 1, 0), (129, 2, 1, 0), (257, 2, 4, 0)]


BIG = (4096, 1, 2048, 0)        # the LDS and register limit: 64 points a lane, 96 KB of LDS

@functools.lru_cache(maxsize=None)
def sweep_def(L, F, step, seed):
    s = sweep_system(L, F, seed)
    return tm_def(s["ref"], s["xyz"], step=step)


@pytest.mark.parametrize("case", SWEEP + [BIG], ids=lambda c: "L%d-F%d-step%d" % c[:3])
def test_sweep_systems_keep_their_decision_margin(case):
    got = sweep_def(*case)
    print(f"L = {case[0]}, F = {case[1]}: decision margin {got['margin']:.3g} A, tm {got['tm64'].min():.3f} .. {got['tm64'].max():.3f}, "
          f"global fit alone {got['first'].min():.3f} .. {got['first'].max():.3f}")
    assert got["margin"] >= MARGIN_CAP
    assert np.isfinite(got["tm64"]).all() and (got["tm64"] > 0).all() and (got["tm64"] <= 1).all()
    assert (got["tm64"] >= got["first"]).all()


# ------------------------------------------------------------------ the host side of pesto_amd.tmscore
def test_arguments_raise_before_any_launch():
    from pesto_amd import tmscore as T
    m = object()                # no handle: the checks must come first
    y, x = np.zeros((6, 3), np.float32), np.zeros((4, 6, 3), np.float32)
    nan_ref = y.copy()
    nan_ref[2, 0] = np.inf
    bad = (dict(xyz=x[:, :5]), dict(xyz=x[:, :, :2]), dict(xyz_ref=np.zeros((2, 6, 3), np.float32)), dict(sel=[0, 6, 1]), dict(sel=[0, 1]),
           dict(sel=np.ones(5, bool)), dict(sel=np.zeros(6)), dict(sel=[-1, 0, 1]), dict(step=0), dict(step=1.5), dict(n_iter=0), dict(n_iter=1025),
           dict(scale=0.0), dict(scale=np.inf), dict(scale=np.nan), dict(norm_len=0), dict(norm_len=np.nan), dict(norm_len=[1, 2]), dict(d0=0.0),
           dict(d0=-1.0), dict(d0=np.inf), dict(sizes=[3, 3]), dict(sizes=[3, 2], xyz=x[:1]), dict(sizes=[6, 0], xyz=x[:1]),
           dict(sizes=[4, 2], xyz=x[:1]), dict(sizes=[3, 3], xyz=x[:1], sel=[3, 4, 5, 0, 1, 2]), dict(sizes=[3, 3], xyz=x[:1], d0=[1, 2, 3]),
           dict(xyz_ref=nan_ref), dict(xyz_ref=nan_ref, sel=[1, 2, 3]))
    for kw in bad:
        args = dict(xyz_ref=y, xyz=x, model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            T.tm_score(**args)
    with pytest.raises(ValueError, match="one model"):
        T.tm_score(y, x, sizes=[3, 3], model=m)
    with pytest.raises(ValueError, match="grouped"):
        T.tm_score(y, x[:1], [3, 4, 5, 0, 1, 2], sizes=[3, 3], model=m)
    with pytest.raises(ValueError, match="4096"):
        T.tm_score(np.zeros((4097, 3), np.float32), np.zeros((1, 4097, 3), np.float32), model=m)
    long = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 23 + 1, 6, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="frames"):
        T.tm_score(y, long, model=m)
    with pytest.raises(ValueError):
        T.gdt(y, x, [0, 1], model=m)
    with pytest.raises(ValueError):
        T.tm_ca(y, x, np.array(["CA"] * 6), sel=[0, 1, 2], model=m)
    with pytest.raises(ValueError):
        T.tm_ca(y, x, np.array(["CA", "CA", "N", "C", "O", "CB"]), model=m)
    with pytest.raises(ValueError):
        T.structure_tmscore(dict(xyz=y, name=np.array(["CA"] * 6), resid=np.arange(6)), dict(xyz=y, name=np.array(["CA"] * 6), resid=np.arange(6)), sel=[0])


def test_new_symbols_are_declared_exported_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_tmscore_last_error", "pesto_tmscore"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.pesto_tmscore_last_error.restype is not None
    assert int(re.search(r"PESTO_TMSCORE_MAX_FRAMES = 1 << (\d+)", hdr).group(1)) == 23
    assert int(re.search(r"PESTO_TMSCORE_MAX_LENGTH = (\d+)", hdr).group(1)) == 4096
    assert int(re.search(r"PESTO_TMSCORE_MAX_ITER = (\d+)", hdr).group(1)) == 1024
    assert int(re.search(r"PESTO_TMSCORE_MAX_RAISE = (\d+)", hdr).group(1)) == MAX_RAISE
    import pesto_amd
    from pesto_amd import tmscore
    assert tmscore.MAX_FRAMES == 2 ** 23 and tmscore.MAX_LENGTH == 4096 and tmscore.MAX_ITER == 1024 and tmscore.MAX_RAISE == MAX_RAISE
    assert pesto_amd.tm_score is tmscore.tm_score and pesto_amd.gdt is tmscore.gdt and pesto_amd.tm_ca is tmscore.tm_ca
    assert pesto_amd.structure_tmscore is tmscore.structure_tmscore and pesto_amd.tmscore is tmscore
    assert tmscore.TMScore._fields == ("tm", "gdt_ts", "gdt_ha", "counts", "rmsd", "seed", "rotation", "translation")
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_tmscore.hip")).read()
    assert "asm" not in src and "atomicAdd" not in src                  # plain C++: no inline assembly, no sums through atomics
    assert "k_fit_rmsd<NT>" in src and "kabsch_fit_wave" in src         # the RMSD and the fit are pesto_fit.h's, not restated
    fit = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_fit.h")).read()
    assert fit.count("kabsch_rotation(H") == 2 and "pesto_tmscore.hip" in open(os.path.join(ROOT, "pesto_amd", "csrc", "build.py")).read()
    assert "tmscore" in open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_call.h")).read().split("#pragma once")[0]
