#!/usr/bin/env python
"""Generate the ranking golden (tests/golden/ranking.npz) from scikit-learn's own functions (build container only, on the CPU; nothing
under tests/ needs sklearn at run time). The yardstick is sklearn 1.7.2 as installed there - the functions the reference's evaluation
notebooks (interface_ppi_benchmark.ipynb, interface_type_evaluation.ipynb, interface_ppi_confidence.ipynb,
interfaceome/eukaryotic_protein_complexes_scoring_analysis.ipynb) and its roc_auc_score (src/scoring.py) call.

    python tests/golden/make_ranking_golden.py

Cases (a column is one (segment, class) pair, numbered s * C + c):
  pdbs53_logits, pdbs53_bfactor, synth     the inputs of tests/golden/eval_scores.npz, read from there (not copied): the 53 chains of
                                           pdbs_test (model probabilities / 2-decimal predictions with heavy ties) and the synthetic
                                           set with its R = 20,000 segment
  pdbs53_logits_pool, pdbs53_bfactor_pool  the same rows as ONE column of 16,825 rows, as the notebooks pool them
  edge          one class, segments of 1, 2, T - 1, T, T + 1 and 2 T + 1 rows (T = 2048, the keys one workgroup handles per radix pass),
                then: all scores tied; all positive; all negative; +0.0 and -0.0 mixed; denormals, negative scores and neighbours in the
                last mantissa bit; p = 0.5 exactly among its neighbours (the rint rule of F1)
  cols255, cols256, cols257                that many columns of 3 rows (51 x 5, 64 x 4, 257 x 1): the column id reaches the next byte
  cols128, cols129                         32 x 4 and 43 x 3 columns of 3 rows: the key grows from 40 to 41 bits, the sort from 5 to 6 passes
Recorded per case: off0, thr, tps, fps (every distinct threshold: _binary_clf_curve per column), off1 and keep (the rows of those that
roc_curve keeps with drop_intermediate=True), counts [S, 6, C] (P, N, TP, FP of rint(p), K, K_roc), scores [S, 3, C] (roc_auc_score,
auc(recall, precision) of precision_recall_curve, f1_score; NaN where roc_auc_score raises and, by this library's rule, for pr_auc without
a positive), edges and hist [S, C, B, 2] (np.histogram per label value). The float64 rate arrays are not recorded: they are quotients of
the recorded integers, and this script asserts that sklearn's own arrays equal those quotients exactly, as restated in the tests and as
pesto_amd.ranking assembles them on the host (roc_points, pr_points, auc). It also asserts that the NumPy
restatement of tests/test_ranking_fixture.py reproduces every recorded array (the areas within K 2^-50) before it writes."""
import os
import sys
import warnings

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import sklearn  # noqa: E402
from sklearn import metrics  # noqa: E402
from sklearn.metrics._ranking import _binary_clf_curve  # noqa: E402

import test_ranking_fixture as T  # noqa: E402
from pesto_amd import ranking as R  # noqa: E402

SKLEARN = "1.7.2"


def edge_case(rng):
    segs, names = [], []

    def add(name, y, p):
        names.append(name)
        segs.append((np.asarray(y, np.uint8), np.asarray(p, np.float32)))

    for n in (1, 2, T.TILE - 1, T.TILE, T.TILE + 1, 2 * T.TILE + 1):
        p = np.round(rng.random(n), 3).astype(np.float32) if n > 2 else rng.random(n).astype(np.float32)      # 3 decimals: ties
        add(f"n{n}", rng.random(n) < 0.3, p)
    add("tied", rng.random(40) < 0.5, np.full(40, 0.25))
    add("all_pos", np.ones(50), rng.random(50))
    add("all_neg", np.zeros(50), rng.random(50))
    add("zeros", rng.random(30) < 0.5, np.where(rng.random(30) < 0.5, 0.0, -0.0))
    tiny = np.finfo(np.float32).tiny
    base = np.array([1.0, -1.0, 0.75, -3.5, 7.25, -12.0, tiny, -tiny, 1e-42, -1e-42, 1.4e-45, -1.4e-45, 0.0, -0.0], np.float32)
    near = np.concatenate([np.nextafter(base, np.float32(np.inf)), np.nextafter(base, np.float32(-np.inf))])
    t = np.concatenate([base, near, base[:8], rng.normal(0, 4, 60).astype(np.float32)]).astype(np.float32)
    add("tiny", rng.random(t.size) < 0.4, rng.permutation(t))
    h = np.concatenate([np.full(6, 0.5), np.nextafter(np.float32(0.5), np.float32([0, 1, 0, 1])), [1.5, 2.5, -0.5, -0.75, 0.25, 0.75]]).astype(np.float32)
    add("half", rng.random(h.size) < 0.5, rng.permutation(h))
    y = np.concatenate([s[0] for s in segs])[:, None]
    p = np.concatenate([s[1] for s in segs])[:, None]
    offsets = np.concatenate([[0], np.cumsum([s[0].size for s in segs])]).astype(np.int32)
    return y, p, offsets, np.array(names, "S")


def cols_case(rng, S, C):
    y = (rng.random((3 * S, C)) < 0.5).astype(np.uint8)
    p = np.round(rng.random((3 * S, C)), 1).astype(np.float32)            # one decimal: ties inside a column of 3
    return y, p, (3 * np.arange(S + 1)).astype(np.int32)


def sklearn_column(y, p, edges):
    """what sklearn gives for one column, with the assertions that tie the recorded integers to its public float64 arrays"""
    fps, tps, thr = _binary_clf_curve(y, p)
    assert np.array_equal(fps, np.rint(fps)) and np.array_equal(tps, np.rint(tps))
    tps_i, fps_i = tps.astype(np.int64), fps.astype(np.int64)
    P, N = int(tps_i[-1]), int(fps_i[-1])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        full = metrics.roc_curve(y, p, drop_intermediate=False)
        kept = metrics.roc_curve(y, p, drop_intermediate=True)
        pr = metrics.precision_recall_curve(y, p)
    for got, want in zip(T.roc_def(thr.astype(np.float32), tps_i, fps_i), full):
        assert np.array_equal(got, want, equal_nan=True)
    # the kept rows: those of the full curve whose thresholds survive (the thresholds are distinct)
    keep = np.nonzero(np.isin(thr, kept[2][1:]))[0]
    assert keep.size == kept[2].size - 1
    for got, want in zip(T.roc_def(thr[keep].astype(np.float32), tps_i[keep], fps_i[keep]), kept):
        assert np.array_equal(got, want, equal_nan=True)
    for got, want in zip(T.pr_def(thr.astype(np.float32), tps_i, fps_i), pr):
        assert np.array_equal(got, want)
    # the module's own host-side assembly and its auc against sklearn's arrays (the tests compare them with roc_def / pr_def)
    for got, want in zip(R.roc_points(thr[keep].astype(np.float32), tps_i[keep], fps_i[keep]), kept):
        assert np.array_equal(got, want, equal_nan=True)
    mine = R.pr_points(thr.astype(np.float32), tps_i, fps_i)
    for got, want in zip(mine, pr):
        assert np.array_equal(got, want)
    assert R.auc(mine[1], mine[0]) == metrics.auc(pr[1], pr[0])
    q = np.rint(p) != 0
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        try:
            roc = metrics.roc_auc_score(y, p)            # one label only: NaN with a warning (a ValueError before sklearn 1.6)
        except ValueError:
            roc = np.nan
    assert np.isnan(roc) == (not (P and N))
    pr_auc = metrics.auc(pr[1], pr[0]) if P else np.nan
    f1 = metrics.f1_score(y, q, zero_division=0)
    TP, FP = int((q & (y != 0)).sum()), int((q & (y == 0)).sum())
    hist = np.stack([np.histogram(p[y == v], bins=edges)[0] for v in (0, 1)], 1)
    return (thr.astype(np.float32), tps_i, fps_i, keep, np.array([P, N, TP, FP, thr.size, keep.size], np.int64),
            np.array([roc, pr_auc, f1], np.float64), hist.astype(np.int64))


def record(out, name, y, p, offsets, edges):
    S, C = offsets.size - 1, y.shape[1]
    off0, off1, thr, tps, fps, keep = [0], [0], [], [], [], []
    counts, sc, hist = np.zeros((S, 6, C), np.int64), np.zeros((S, 3, C), np.float64), np.zeros((S, C, edges.size - 1, 2), np.int64)
    for col, (yc, pc) in enumerate(T.columns(y, p, offsets)):
        t, a, b, k, cn, s, h = sklearn_column(yc, pc, edges)
        thr.append(t); tps.append(a); fps.append(b); keep.append(k + off0[-1])
        off0.append(off0[-1] + t.size); off1.append(off1[-1] + k.size)
        counts[col // C, :, col % C], sc[col // C, :, col % C], hist[col // C, col % C] = cn, s, h
    thr = np.concatenate(thr)
    thr = np.where(thr == 0, np.float32(0), thr).astype(np.float32)          # -0.0 and +0.0 are one threshold: recorded as +0.0
    out.update({f"{name}_off0": np.array(off0, np.int32), f"{name}_off1": np.array(off1, np.int32), f"{name}_thr": thr,
                f"{name}_tps": np.concatenate(tps).astype(np.int32), f"{name}_fps": np.concatenate(fps).astype(np.int32),
                f"{name}_keep": np.concatenate(keep).astype(np.int32), f"{name}_counts": counts, f"{name}_scores": sc,
                f"{name}_edges": edges.astype(np.float32), f"{name}_hist": hist})


def main():
    assert sklearn.__version__ == SKLEARN, sklearn.__version__
    rng = np.random.default_rng(20240607)
    out = {"sklearn_version": np.array(SKLEARN)}
    y, p, offsets, names = edge_case(rng)
    out.update(edge_y=y, edge_p=p, edge_offsets=offsets, edge_segments=names)
    for S, C in ((51, 5), (64, 4), (257, 1), (32, 4), (43, 3)):
        y, p, offsets = cols_case(rng, S, C)
        out.update({f"cols{S * C}_y": y, f"cols{S * C}_p": p, f"cols{S * C}_offsets": offsets})
    unit = np.linspace(0.0, 1.0, 11).astype(np.float32)                      # the notebooks' confidence bins
    wide = np.array([-20, -1, -1e-40, 0, 1e-40, 0.25, 0.5, 0.75, 1, 20], np.float32)
    path = os.path.join(OUT, "ranking.npz")
    np.savez_compressed(path, **out)                                         # (T.inputs reads the new cases from the file)
    for name in T.CASES:
        yy, pp, oo = (out[name + "_y"], out[name + "_p"], out[name + "_offsets"]) if name in T.NEW_CASES else T.inputs(name)
        record(out, name, yy, pp, oo, wide if name == "edge" else unit)
    np.savez_compressed(path, **out)
    # the restatement reproduces what was recorded
    g = np.load(path)
    for name in T.CASES:
        d = T.case_def(name)
        for key in ("off0", "tps", "fps", "off1", "keep", "counts", "hist"):
            assert np.array_equal(d[key], g[f"{name}_{key}"].astype(np.int64)), (name, key)
        assert np.array_equal(d["thr"].view(np.uint32), g[name + "_thr"].view(np.uint32)), name
        rec, K = g[name + "_scores"], d["counts"][:, 4, :]
        assert np.array_equal(np.isnan(d["scores"]), np.isnan(rec)), name
        err = np.abs(d["scores"] - rec)
        assert np.all(np.isnan(err[:, :2]) | (err[:, :2] <= T.area_tolerance(K)[:, None, :])) and np.array_equal(d["scores"][:, 2], rec[:, 2]), name
        print(f"{name}: {d['off0'].size - 1} columns, {d['thr'].size} thresholds, {d['keep'].size} kept, max area deviation "
              f"{np.nanmax(err[:, :2]) if np.isfinite(err[:, :2]).any() else 0.0:.3g}")
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) <= 1_000_000


if __name__ == "__main__":
    main()
