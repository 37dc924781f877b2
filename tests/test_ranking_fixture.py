"""CPU checks of the ranking fixture (tests/golden/make_ranking_golden.py) and of the host side of pesto_amd.ranking: a NumPy
restatement of the definitions (stable descending sort, group ends, cumulative sums, the drop_intermediate rule, the trapezoid)
reproduces the outputs recorded from sklearn - thresholds, tps, fps, the kept points and the histograms exactly, the areas within their
rounding - the module's host-side assembly of the rates and its auc equal sklearn's float64 arrays exactly, bad arguments raise ValueError
before any launch, and the header's new symbols are exported and bound. The restatement is the yardstick of the GPU tests
(tests/test_ranking.py); the generator records sklearn's outputs after asserting that the restatement agrees with them."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT, golden

TILE = 2048                             # pesto_radix.h: RADIX_TILE, the keys one workgroup handles per radix pass (ranking.RADIX_TILE)
EVAL_CASES = ["pdbs53_logits", "pdbs53_bfactor", "synth"]          # inputs in eval_scores.npz
POOLED = ["pdbs53_logits", "pdbs53_bfactor"]                       # recorded once more as one column of 16,825 rows (<case>_pool)
NEW_CASES = ["edge", "cols255", "cols256", "cols257", "cols128", "cols129"]     # inputs in ranking.npz itself
CASES = EVAL_CASES + [c + "_pool" for c in POOLED] + NEW_CASES


def inputs(name):
    """(y uint8 [R, C], p float32 [R, C], offsets int32 [S + 1]) of a case"""
    if name in NEW_CASES:
        g = golden("ranking")
        return g[name + "_y"], g[name + "_p"], g[name + "_offsets"]
    g = golden("eval_scores")
    base = name[:-5] if name.endswith("_pool") else name
    y, p = g[base + "_y"], g[base + "_p"]
    return y, p, (np.array([0, y.shape[0]], np.int32) if name.endswith("_pool") else g[base + "_offsets"])


def columns(y, p, offsets):
    """the (y [R_s], p [R_s]) of every column, in the order s * C + c"""
    return [(y[offsets[s]:offsets[s + 1], c], p[offsets[s]:offsets[s + 1], c]) for s in range(offsets.size - 1) for c in range(y.shape[1])]


# ------------------------------------------------------------------ the definitions (NumPy)
def curve_def(y, p):
    """(thr float32 [K], tps int64 [K], fps int64 [K]) of one column: the distinct scores in descending order, the positives and the
    negatives at or above each (sklearn's _binary_clf_curve); -0.0 is +0.0"""
    p = np.where(p == 0, np.float32(0), p).astype(np.float32)
    order = np.argsort(-p, kind="stable")
    ps, ys = p[order], (y[order] != 0).astype(np.int64)
    ends = np.r_[np.nonzero(np.diff(ps))[0], ps.size - 1]
    tps = np.cumsum(ys)[ends]
    return ps[ends], tps, 1 + ends - tps


def keep_def(tps, fps):
    """the rows roc_curve keeps with drop_intermediate=True: the ends and where the second difference of fps or of tps is not zero"""
    if tps.size <= 2:
        return np.arange(tps.size)
    return np.nonzero(np.r_[True, np.logical_or(np.diff(fps, 2), np.diff(tps, 2)), True])[0]


def trapezoid(x, y):
    """sklearn's auc: the trapezoid of y over a monotone x in float64, positive for a falling x too"""
    dx = np.diff(x)
    return float((-1.0 if np.any(dx < 0) else 1.0) * (dx * (y[1:] + y[:-1]) / 2.0).sum())


def roc_def(thr, tps, fps):
    """(fpr, tpr, thresholds) as roc_curve returns them for these rows"""
    t, f = np.r_[0, tps].astype(np.float64), np.r_[0, fps].astype(np.float64)
    with np.errstate(invalid="ignore"):
        return f / f[-1], t / t[-1], np.r_[np.float32(np.inf), thr].astype(np.float32)


def pr_def(thr, tps, fps):
    """(precision, recall, thresholds) as precision_recall_curve returns them"""
    t = tps.astype(np.float64)
    precision = t / (tps + fps)
    recall = t / t[-1] if tps[-1] else np.ones_like(t)
    return np.r_[precision[::-1], 1.0], np.r_[recall[::-1], 0.0], thr[::-1]


def scores_def(y, p):
    """(counts int64 [6], scores float64 [3]) of one column: P, N, TP, FP (q = rint(p) != 0), K, K_roc; roc_auc (NaN unless both labels
    occur), pr_auc (NaN without a positive), f1 (0 for an empty denominator)"""
    thr, tps, fps = curve_def(y, p)
    P, N = int(tps[-1]), int(fps[-1])
    q, yb = np.rint(p) != 0, y != 0
    TP, FP = int((q & yb).sum()), int((q & ~yb).sum())
    keep = keep_def(tps, fps)
    fpr, tpr, _ = roc_def(thr[keep], tps[keep], fps[keep])
    pre, rec, _ = pr_def(thr, tps, fps)
    den = 2 * TP + FP + (P - TP)
    sc = [trapezoid(fpr, tpr) if P and N else np.nan, trapezoid(rec, pre) if P else np.nan, 2 * TP / den if den else 0.0]
    return np.array([P, N, TP, FP, thr.size, keep.size], np.int64), np.array(sc, np.float64)


def hist_def(y, p, edges):
    """int64 [B, 2]: np.histogram(p[y == v], bins=edges) for v = 0, 1"""
    return np.stack([np.histogram(p[(y != 0) == v], bins=edges)[0] for v in (False, True)], 1).astype(np.int64)


_defs = {}


def case_def(name):
    """the restatement of a whole case, computed once: dict with off0 [ncol + 1], thr, tps, fps (mode 0), off1, keep (mode 1: rows of the
    mode-0 arrays), counts [S, 6, C], scores [S, 3, C], edges and hist [S, C, B, 2]"""
    if name not in _defs:
        y, p, offsets = inputs(name)
        S, C = offsets.size - 1, y.shape[1]
        edges = golden("ranking")[name + "_edges"]
        off0, off1, thr, tps, fps, keep = [0], [0], [], [], [], []
        counts, sc, hist = np.zeros((S, 6, C), np.int64), np.zeros((S, 3, C), np.float64), np.zeros((S, C, edges.size - 1, 2), np.int64)
        for col, (yc, pc) in enumerate(columns(y, p, offsets)):
            t, a, b = curve_def(yc, pc)
            k = keep_def(a, b)
            thr.append(t); tps.append(a); fps.append(b); keep.append(k + off0[-1])
            off0.append(off0[-1] + t.size); off1.append(off1[-1] + k.size)
            counts[col // C, :, col % C], sc[col // C, :, col % C] = scores_def(yc, pc)
            hist[col // C, col % C] = hist_def(yc, pc, edges)
        _defs[name] = dict(off0=np.array(off0, np.int64), off1=np.array(off1, np.int64), thr=np.concatenate(thr), tps=np.concatenate(tps),
                           fps=np.concatenate(fps), keep=np.concatenate(keep), counts=counts, scores=sc, edges=edges, hist=hist)
    return _defs[name]


def area_tolerance(K):
    """K 2^-50: K trapezoid terms of at most 1 each, a few float64 roundings per term in either sum"""
    return K * 2.0 ** -50


# ------------------------------------------------------------------ the fixture
def test_fixture_loads_and_holds_the_cases_the_issue_lists():
    g = golden("ranking")
    assert str(g["sklearn_version"]) == "1.7.2"
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "ranking.npz")) <= 1_000_000
    for name in CASES:
        for key in ("off0", "thr", "tps", "fps", "off1", "keep", "counts", "scores", "edges", "hist"):
            assert f"{name}_{key}" in g.files, (name, key)
    y, p, off = inputs("edge")
    lengths = np.diff(off).tolist()
    assert y.shape[1] == 1 and lengths[:6] == [1, 2, TILE - 1, TILE, TILE + 1, 2 * TILE + 1]
    names = [n.decode() for n in g["edge_segments"]]
    assert names[6:] == ["tied", "all_pos", "all_neg", "zeros", "tiny", "half"] and len(names) == len(lengths)
    seg = {n: (y[off[i]:off[i + 1], 0], p[off[i]:off[i + 1], 0]) for i, n in enumerate(names)}
    assert np.unique(seg["tied"][1]).size == 1 and seg["all_pos"][0].all() and not seg["all_neg"][0].any()
    z = seg["zeros"][1]
    assert (z == 0).all() and np.signbit(z).any() and not np.signbit(z).all()
    t = seg["tiny"][1]
    assert ((t != 0) & (np.abs(t) < np.finfo(np.float32).tiny)).any() and (t < 0).any()
    assert np.any(np.diff(np.sort(t).view(np.int32)) == 1)                # neighbours in the last mantissa bit
    assert (seg["half"][1] == 0.5).any()
    # 255 .. 257 columns: the column id reaches the next byte; 128 / 129: the sort goes from 5 to 6 radix passes (40 key bits to 41)
    for n, ncol in (("cols255", 255), ("cols256", 256), ("cols257", 257), ("cols128", 128), ("cols129", 129)):
        yy, pp, oo = inputs(n)
        assert (oo.size - 1) * yy.shape[1] == ncol and np.all(np.diff(oo) == 3)
    assert max(np.diff(inputs("synth")[2])) == 20000


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_recorded_sklearn_outputs(name):
    g, d = golden("ranking"), case_def(name)
    for key in ("off0", "tps", "fps", "off1", "keep", "counts", "hist"):
        assert np.array_equal(d[key], g[f"{name}_{key}"].astype(np.int64)), (name, key)
    assert np.array_equal(d["thr"].view(np.uint32), g[name + "_thr"].view(np.uint32))
    rec, K = g[name + "_scores"], d["counts"][:, 4, :]
    assert np.array_equal(np.isnan(d["scores"]), np.isnan(rec))
    for row in (0, 1):
        err = np.abs(d["scores"][:, row, :] - rec[:, row, :])
        assert np.all(np.isnan(err) | (err <= area_tolerance(K))), (name, row, np.nanmax(err))
    assert np.array_equal(d["scores"][:, 2, :], rec[:, 2, :])


def test_pooled_counts_are_the_sums_of_the_chains():
    for base in POOLED:
        per, pool = case_def(base)["counts"], case_def(base + "_pool")["counts"]
        assert np.array_equal(per[:, :4, :].sum(0), pool[0, :4, :])
        assert np.array_equal(case_def(base)["hist"].sum(0), case_def(base + "_pool")["hist"][0])


# ------------------------------------------------------------------ the host side of pesto_amd.ranking
@pytest.mark.parametrize("name", ["pdbs53_bfactor", "pdbs53_logits_pool", "edge"])
def test_host_assembly_equals_the_definitions_exactly(name):
    from pesto_amd import ranking as R
    d = case_def(name)
    for col in range(d["off0"].size - 1):
        rows = slice(d["off0"][col], d["off0"][col + 1])
        for sel in (np.arange(rows.start, rows.stop), d["keep"][d["off1"][col]:d["off1"][col + 1]]):
            thr, tps, fps = d["thr"][sel], d["tps"][sel], d["fps"][sel]
            for got, want in zip(R.roc_points(thr, tps, fps), roc_def(thr, tps, fps)):
                assert got.dtype == want.dtype and np.array_equal(got, want, equal_nan=True)
        thr, tps, fps = d["thr"][rows], d["tps"][rows], d["fps"][rows]
        pre, rec, t = R.pr_points(thr, tps, fps)
        for got, want in zip((pre, rec, t), pr_def(thr, tps, fps)):
            assert got.dtype == want.dtype and np.array_equal(got, want)
        assert R.auc(rec, pre) == trapezoid(rec, pre)


def test_auc_follows_sklearns_direction_rule():
    from pesto_amd import ranking as R
    assert R.auc([0, 1, 2], [0, 1, 1]) == 1.5 and R.auc([2, 1, 0], [1, 1, 0]) == 1.5
    for x, y in (([0, 2, 1], [0, 1, 2]), ([0], [1]), ([0, 1], [0, 1, 2])):
        with pytest.raises(ValueError):
            R.auc(x, y)


def test_bad_arguments_raise_before_any_launch():
    from pesto_amd import ranking as R
    y, p = np.array([0, 1, 1, 0], np.uint8), np.array([0.1, 0.9, 0.4, 0.4], np.float32)
    m = object()                                        # never reached: a launch would fail on it
    bad = [dict(p=p.astype(np.float64)), dict(y=y.astype(np.float32)), dict(y=y[:3]), dict(y=y * 2), dict(y=np.array([0, 1, -1, 0])),
           dict(p=p.reshape(2, 2, 1), y=y.reshape(2, 2, 1)), dict(p=p[:0], y=y[:0]), dict(offsets=[0, 2, 2, 4]), dict(offsets=[0, 5]),
           dict(offsets=[1, 4]), dict(offsets=[0.0, 4.0]), dict(offsets=[0]), dict(p=np.zeros((2, 1025), np.float32), y=np.zeros((2, 1025), np.uint8))]
    for kw in bad:
        args = dict(y=y, p=p, model=m)
        args.update(kw)
        for fn in (R.scores, R.roc_curve, R.precision_recall_curve, R.curves, R.roc_auc, R.pr_auc, R.f1):
            with pytest.raises(ValueError):
                fn(**args)
        with pytest.raises(ValueError):
            R.confidence_histogram(edges=[0.0, 0.5, 1.0], **args)
    for edges in ([0.0], [0.0, 0.0], [0.0, 1.0, 0.5], [0.0, np.nan], [0.0, 1e-46]):
        with pytest.raises(ValueError):
            R.confidence_histogram(y, p, edges, model=m)
    with pytest.raises(ValueError, match="columns"):    # 2^24 columns: a workgroup per column would pass the grid limit
        R.scores(np.zeros((2 ** 14, 1024), np.uint8), np.zeros((2 ** 14, 1024), np.float32), offsets=np.arange(2 ** 14 + 1), model=m)
    for cap in (-1, 2 ** 31):
        with pytest.raises(ValueError):
            R.curves(y, p, capacity=cap, model=m)


def test_new_symbols_are_declared_exported_and_bound():
    from pesto_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    new = ["pesto_rank_last_error", "pesto_rank_scores", "pesto_rank_curves", "pesto_rank_histogram"]
    lib = _lib.load()
    for name in new:
        assert re.search(rf"\b{name}\s*\(", hdr), name
        assert name in _lib.ABI_SYMBOLS and hasattr(lib, name)
        assert getattr(lib, name).argtypes is not None
    assert lib.pesto_rank_last_error.restype is not None
    assert int(re.search(r"PESTO_RANK_TILE = (\d+)", hdr).group(1)) == TILE
    import pesto_amd
    from pesto_amd import ranking
    assert ranking.RADIX_TILE == TILE and pesto_amd.roc_curve is ranking.roc_curve and pesto_amd.ranking is ranking
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_radix.h")).read()
    build_py = open(os.path.join(ROOT, "pesto_amd", "csrc", "build.py")).read()
    assert "RADIX_TILE = PESTO_RANK_TILE" in src and "pesto_rank.hip" in build_py and "pesto_radix.h" in build_py
