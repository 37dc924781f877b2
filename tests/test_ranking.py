"""GPU tests of pesto_amd.ranking (pesto_rank.hip) against the NumPy restatement of tests/test_ranking_fixture.py, which reproduces the
sklearn outputs recorded in tests/golden/ranking.npz: thresholds by value, tps, fps, offsets, counts and histograms exactly (so the
float64 rates are exact too), through host arrays and ROCm tensors; f1 within one ulp and roc_auc / pr_auc within K 2^-50 of sklearn's
recorded values; float32(roc_auc) bit for bit the auc row of evaluate.bc_scores_batch; the same bits from call to call; the capacity
protocol; mode 1 against mode 0 thinned; 53 chains batched, one by one and pooled; a non-finite score raises and the next call succeeds."""
import numpy as np
import pytest

from conftest import golden
from test_ranking_fixture import (CASES, EVAL_CASES, NEW_CASES, POOLED, area_tolerance, case_def, inputs, keep_def, pr_def, roc_def)

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def place(on_device, *arrays):
    return [dev(a) if on_device else a for a in arrays]


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def check_curve(got, d, rows, offsets, on_device):
    off, thr, tps, fps = got
    assert all(v.is_cuda for v in got) if on_device else all(isinstance(v, np.ndarray) for v in got)
    assert host(off).dtype == np.int64 and host(thr).dtype == np.float32 and host(tps).dtype == np.int64 and host(fps).dtype == np.int64
    assert np.array_equal(host(off), offsets)
    assert np.array_equal(host(thr), d["thr"][rows]) and np.array_equal(host(tps), d["tps"][rows]) and np.array_equal(host(fps), d["fps"][rows])


def check_scores(got, d, recorded):
    counts, sc = host(got["counts"]), host(got["scores"])
    assert counts.dtype == np.int64 and sc.dtype == np.float64
    assert np.array_equal(counts, d["counts"])
    assert np.array_equal(np.isnan(sc), np.isnan(recorded))
    K = d["counts"][:, 4, :]
    for row in (0, 1):
        err = np.abs(sc[:, row, :] - recorded[:, row, :])
        print("max deviation of", ["roc_auc", "pr_auc"][row], np.nanmax(err) if np.isfinite(err).any() else 0.0, "allowed", area_tolerance(K).min())
        assert np.all(np.isnan(err) | (err <= area_tolerance(K)))
    assert np.all(np.abs(sc[:, 2, :] - recorded[:, 2, :]) <= np.spacing(recorded[:, 2, :]))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", CASES)
def test_curves_scores_and_histograms_equal_the_definitions(name, on_device):
    from pesto_amd import ranking as R
    g, d = golden("ranking"), case_def(name)
    y, p, offsets = inputs(name)
    yd, pd = place(on_device, y, p)
    full = R.curves(yd, pd, False, offsets)
    check_curve(full, d, slice(None), d["off0"], on_device)
    kept = R.curves(yd, pd, True, offsets)
    check_curve(kept, d, d["keep"], d["off1"], on_device)
    # mode 1 is mode 0 thinned by the restatement's rule
    o, tps, fps = host(full[0]), host(full[2]), host(full[3])
    thin = np.concatenate([o[c] + keep_def(tps[o[c]:o[c + 1]], fps[o[c]:o[c + 1]]) for c in range(o.size - 1)])
    assert all(np.array_equal(host(k), host(f)[thin]) for k, f in zip(kept[1:], full[1:]))
    sc = R.scores(yd, pd, offsets)
    check_scores(sc, d, g[name + "_scores"])
    hist = R.confidence_histogram(yd, pd, d["edges"], offsets)
    assert (hist.is_cuda if on_device else isinstance(hist, np.ndarray)) and host(hist).dtype == np.int64
    assert np.array_equal(host(hist), d["hist"])
    # the same bits from call to call
    again = R.curves(yd, pd, False, offsets), R.curves(yd, pd, True, offsets), R.scores(yd, pd, offsets), R.confidence_histogram(yd, pd, d["edges"], offsets)
    assert all(same_bits(u, v) for u, v in zip(full + kept, again[0] + again[1]))
    assert same_bits(sc["counts"], again[2]["counts"]) and same_bits(sc["scores"], again[2]["scores"]) and same_bits(hist, again[3])


@pytest.mark.parametrize("name", EVAL_CASES + NEW_CASES)
def test_float32_roc_auc_has_the_bits_of_bc_scoring(name):
    from pesto_amd import evaluate as E
    from pesto_amd import ranking as R
    y, p, offsets = inputs(name)
    model = E._scoring_model(0)
    ys, ps = [y[offsets[s]:offsets[s + 1]] for s in range(offsets.size - 1)], [p[offsets[s]:offsets[s + 1]] for s in range(offsets.size - 1)]
    bc = E.bc_scores_batch(model, ys, ps)[:, 6, :]
    roc = R.roc_auc(y, p, offsets)
    assert roc.shape == bc.shape and np.array_equal(roc.astype(np.float32).view(np.uint32), bc.view(np.uint32))
    if name in POOLED:
        assert np.array_equal(bc.view(np.uint32), golden("eval_scores")[name + "_scores"][:, 6, :].view(np.uint32))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_rates_equal_sklearns_float64_arrays(on_device):
    from pesto_amd import ranking as R
    # several columns: a list per column
    d = case_def("pdbs53_bfactor")
    y, p, offsets = inputs("pdbs53_bfactor")
    yd, pd = place(on_device, y, p)
    for drop, off, sel in ((False, d["off0"], None), (True, d["off1"], d["keep"])):
        got = R.roc_curve(yd, pd, drop, offsets)
        assert isinstance(got, list) and len(got) == off.size - 1
        for col, triple in enumerate(got):
            rows = slice(off[col], off[col + 1]) if sel is None else sel[off[col]:off[col + 1]]
            for a, b in zip(triple, roc_def(d["thr"][rows], d["tps"][rows], d["fps"][rows])):
                assert (a.is_cuda if on_device else isinstance(a, np.ndarray)) and host(a).dtype == b.dtype and np.array_equal(host(a), b, equal_nan=True)
    got = R.precision_recall_curve(yd, pd, offsets)
    for col, triple in enumerate(got):
        rows = slice(d["off0"][col], d["off0"][col + 1])
        for a, b in zip(triple, pr_def(d["thr"][rows], d["tps"][rows], d["fps"][rows])):
            assert host(a).dtype == b.dtype and np.array_equal(host(a), b)
    # one pooled column: arrays, and the thin views of scores
    d = case_def("pdbs53_logits_pool")
    y, p, _ = inputs("pdbs53_logits_pool")
    yd, pd = place(on_device, y[:, 0], p[:, 0])
    k = d["keep"]
    for a, b in zip(R.roc_curve(yd, pd), roc_def(d["thr"][k], d["tps"][k], d["fps"][k])):
        assert np.array_equal(host(a), b)
    pre, rec, thr = R.precision_recall_curve(yd, pd)
    for a, b in zip((pre, rec, thr), pr_def(d["thr"], d["tps"], d["fps"])):
        assert np.array_equal(host(a), b)
    rec_sc = golden("ranking")["pdbs53_logits_pool_scores"][0, :, 0]
    tol = area_tolerance(d["thr"].size)
    assert abs(R.auc(rec, pre) - rec_sc[1]) <= tol and abs(R.pr_auc(yd, pd) - rec_sc[1]) <= tol
    fpr, tpr, _ = R.roc_curve(yd, pd, drop_intermediate=False)
    assert abs(R.auc(fpr, tpr) - rec_sc[0]) <= tol and abs(R.roc_auc(yd, pd) - rec_sc[0]) <= tol
    assert abs(R.f1(yd, pd) - rec_sc[2]) <= np.spacing(rec_sc[2])
    hist = R.confidence_histogram(yd, pd, d["edges"])
    assert tuple(hist.shape) == (d["edges"].size - 1, 2) and np.array_equal(host(hist), d["hist"][0, 0])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("mode", [0, 1])
def test_capacity_too_small_returns_the_count_and_the_repeat_completes(mode, on_device):
    from pesto_amd import _lib
    from pesto_amd import ranking as R
    from pesto_amd.patches import _default_model
    d = case_def("edge")
    y, p, offsets = inputs("edge")
    rows, off = (slice(None), d["off0"]) if mode == 0 else (d["keep"], d["off1"])
    K = int(off[-1])
    model = _default_model(0)
    side = _lib.Side(dev(p) if on_device else p, model._gpu)
    yd, pd = side.put(y, np.uint8), side.put(p, np.float32)
    lib = _lib.load()
    for cap in (0, K - 1, K):
        o, sz = side.empty((off.size,), np.int64), np.zeros(1, np.int64)
        thr, tps, fps = side.empty((cap,), np.float32), side.empty((cap,), np.int64), side.empty((cap,), np.int64)
        for a, fill in ((thr, -7.0), (tps, -7), (fps, -7)):
            if on_device:
                a.fill_(fill)
            else:
                a[...] = fill
        _lib.check(lib.pesto_rank_curves(model.handle, offsets.size - 1, offsets.ctypes.data, 1, side.ptr(yd), side.ptr(pd), mode, cap, side.ptr(o),
                                         side.ptr(thr) if cap else None, side.ptr(tps) if cap else None, side.ptr(fps) if cap else None, sz.ctypes.data,
                                         side.kind, side.stream), lib.pesto_rank_last_error)
        assert int(sz[0]) == K and np.array_equal(host(o), off)
        if cap < K:                                     # nothing is emitted
            assert np.all(host(thr) == -7.0) and np.all(host(tps) == -7) and np.all(host(fps) == -7)
        else:
            assert np.array_equal(host(thr), d["thr"][rows]) and np.array_equal(host(tps), d["tps"][rows]) and np.array_equal(host(fps), d["fps"][rows])
    got = R.curves(yd, pd, bool(mode), offsets, capacity=K - 1)                # the module repeats the call
    assert np.array_equal(host(got[0]), off) and np.array_equal(host(got[1]), d["thr"][rows]) and np.array_equal(host(got[2]), d["tps"][rows])


@pytest.mark.parametrize("base", POOLED)
def test_chains_batched_one_by_one_and_pooled(base):
    from pesto_amd import ranking as R
    d, pool = case_def(base), case_def(base + "_pool")
    y, p, offsets = inputs(base)
    batch_sc, batch_cv, batch_h = R.scores(y, p, offsets), R.curves(y, p, False, offsets), R.confidence_histogram(y, p, d["edges"], offsets)
    o = batch_cv[0]
    for s in range(offsets.size - 1):
        ys, ps = y[offsets[s]:offsets[s + 1]], p[offsets[s]:offsets[s + 1]]
        one = R.scores(ys, ps)
        assert same_bits(one["counts"][0], batch_sc["counts"][s]) and same_bits(one["scores"][0], batch_sc["scores"][s])
        cv = R.curves(ys, ps)
        assert cv[0].tolist() == [0, o[s + 1] - o[s]] and all(same_bits(a, b[o[s]:o[s + 1]]) for a, b in zip(cv[1:], batch_cv[1:]))
        assert same_bits(R.confidence_histogram(ys, ps, d["edges"]), batch_h[s, 0])
    pooled = R.scores(y, p)                             # S = 1: one column of 16,825 rows
    assert np.array_equal(pooled["counts"], pool["counts"]) and np.array_equal(pooled["counts"][0, :4], batch_sc["counts"][:, :4].sum(0))
    cv = R.curves(y, p)
    assert np.array_equal(cv[1], pool["thr"]) and np.array_equal(cv[2], pool["tps"]) and np.array_equal(cv[3], pool["fps"])
    assert np.array_equal(R.confidence_histogram(y, p, d["edges"]), batch_h.sum(0)[0])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("bad", [np.nan, np.inf, -np.inf])
def test_a_non_finite_score_raises_and_the_next_call_succeeds(bad, on_device):
    from pesto_amd import _lib
    from pesto_amd import ranking as R
    d = case_def("cols256")
    y, p, offsets = inputs("cols256")
    q = p.copy()
    q[101, 2] = bad
    yd, pd, qd = place(on_device, y, p, q)
    for call in (lambda: R.scores(yd, qd, offsets), lambda: R.curves(yd, qd, True, offsets), lambda: R.confidence_histogram(yd, qd, d["edges"], offsets)):
        with pytest.raises(_lib.PestoError, match="non-finite") as e:
            call()
        assert e.value.code == -1 and b"non-finite" in _lib.load().pesto_rank_last_error()
    assert np.array_equal(host(R.scores(yd, pd, offsets)["counts"]), d["counts"])
