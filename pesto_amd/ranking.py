"""Ranking curves and pooled scores on the GPU: what the reference's evaluation notebooks take from sklearn.metrics.

interface_ppi_benchmark.ipynb, interface_type_evaluation.ipynb, interface_ppi_confidence.ipynb and
interfaceome/eukaryotic_protein_complexes_scoring_analysis.ipynb pool the residues of hundreds of structures into one column of 10^5 to
10^7 rows and call metrics.roc_curve, metrics.precision_recall_curve with metrics.auc, metrics.f1_score and np.histogram on it. Here
(pesto_rank.hip: one segmented radix sort of 64-bit keys, then integer scans):
    scores                          {"counts" int64 [S, 6, C], "scores" float64 [S, 3, C]}: P, N, TP, FP, K, K_roc; roc_auc, pr_auc, f1
    roc_auc / pr_auc / f1           rows of ``scores``
    roc_curve                       (fpr, tpr, thresholds), metrics.roc_curve with its drop_intermediate
    precision_recall_curve          (precision, recall, thresholds), metrics.precision_recall_curve
    curves                          the integer curves themselves: (offsets int64 [S C + 1], thr float32, tps int64, fps int64)
    auc                             metrics.auc: the trapezoid with sklearn's direction rule (host, float64)
    confidence_histogram            int64 [S, C, B, 2]: np.histogram(p[y == v], bins=edges) per column and label value v
The inputs are evaluate.bc_scoring's: y [R, C] (0 / 1; bool or an integer type) and p float32 [R, C], or [R] for one class; ``offsets``
(int32 [S + 1], from 0 to R, no empty segment) splits the rows into S segments. A column is one (segment, class) pair, numbered
s * C + c; pooled evaluation is one segment. For one column (no offsets, one class) the functions return arrays; otherwise a list with one
entry per column. p decides where a call runs (_lib.Side): ROCm tensors stay on the device (device pointers, torch's current stream, ROCm
tensors out, the rates made by torch on the device); NumPy arrays and CPU tensors are staged. ``model`` lends its device handle; without one
a weightless handle is used. Arguments are checked before any launch (ValueError); a NaN or an infinite score raises PestoError, as sklearn
refuses it. There is no CPU or PyTorch fallback.

tps, fps, the counts and the histograms are exact integers, so fpr, tpr, precision and recall - float64 quotients of them - equal
sklearn's arrays exactly, and thresholds equal the scores they came from (-0.0 is reported as +0.0: the two are one threshold). roc_auc is
(double)u2 / (2 P N) with u2 the integer evaluate.bc_scoring counts over all pairs: rounded to float32 it is that function's auc row bit
for bit. Two NaN rules: roc_auc is NaN unless the column has a positive and a negative; pr_auc is NaN without a positive, where sklearn sets
the recall to 1 with a warning and returns an area that means nothing. Not covered: sample weights, pos_label, average precision.
"""
import numpy as np

from . import _lib
from .trajectory import _model_of

RADIX_TILE = 2048               # PESTO_RANK_TILE: the keys one workgroup handles per radix pass
MAX_CLASSES = 1024
MAX_COLUMNS = 2 ** 24 - 1       # PESTO_RANK_MAX_COLUMNS: S * C, a workgroup per column
COUNT_NAMES = ["P", "N", "TP", "FP", "K", "K_roc"]
SCORE_NAMES = ["roc_auc", "pr_auc", "f1"]


def _dtype_name(a):
    return str(a.dtype).replace("torch.", "")


def _columns(y, p, offsets):
    """(y [R, C], p [R, C], offsets int32 [S + 1], S, C, single) after the argument checks; single: one column, arrays come back"""
    if not hasattr(p, "dtype"):
        p = np.asarray(p, np.float32)
    if not hasattr(y, "dtype"):
        y = np.asarray(y)
    if _dtype_name(p) != "float32":
        raise ValueError(f"p must be float32, got {_dtype_name(p)}")
    if _dtype_name(y) not in ("bool", "uint8", "int8", "int16", "int32", "int64"):
        raise ValueError(f"y must be bool or an integer type, got {_dtype_name(y)}")
    shape = tuple(int(v) for v in p.shape)
    if len(shape) not in (1, 2) or tuple(int(v) for v in y.shape) != shape:
        raise ValueError(f"y and p must both be [R] or [R, C], got {list(y.shape)} and {list(p.shape)}")
    R, C = shape[0], (shape[1] if len(shape) == 2 else 1)
    if R < 1 or not 1 <= C <= MAX_CLASSES or R * C > 2 ** 31 - 1:
        raise ValueError(f"R >= 1, 1 <= C <= {MAX_CLASSES} and R * C <= 2**31 - 1, got R = {R}, C = {C}")
    if _dtype_name(y) != "bool" and bool(((y != 0) & (y != 1)).any()):
        raise ValueError("y must hold 0 and 1 only")
    if offsets is None:
        offs = np.array([0, R], np.int32)
    else:
        o = _lib.host(offsets).reshape(-1)
        if o.size < 2 or not np.issubdtype(o.dtype, np.integer) or o[0] != 0 or o[-1] != R or not np.all(o[1:] > o[:-1]):
            raise ValueError(f"offsets must be integers rising strictly from 0 to {R}")
        offs = np.ascontiguousarray(o, np.int32)
    S = offs.size - 1
    if S * C > MAX_COLUMNS:
        raise ValueError(f"at most 2**24 - 1 columns per call, got {S} * {C}")
    return y.reshape(R, C), p.reshape(R, C), offs, S, C, offsets is None and C == 1


def _placed(y, p, offsets, model):
    y, p, offs, S, C, single = _columns(y, p, offsets)
    model = _model_of(model, p)
    side = _lib.Side(p, model._gpu)
    return side, model.handle, side.put(y != 0, np.uint8), side.put(p, np.float32), offs, S, C, single


def scores(y, p, offsets=None, model=None):
    """{"counts": int64 [S, 6, C], "scores": float64 [S, 3, C]} of every column: counts rows P, N, TP, FP (of q = round(p) half to even,
    as evaluate.bc_scoring), K (distinct thresholds), K_roc (the points roc_curve keeps); scores rows roc_auc, pr_auc =
    auc(recall, precision) of precision_recall_curve, f1 (0.0 for an empty denominator). See the module docstring for the NaN rules."""
    side, h, yd, pd, offs, S, C, _ = _placed(y, p, offsets, model)
    counts, sc = side.empty((S, 6, C), np.int64), side.empty((S, 3, C), np.float64)
    lib = _lib.load()
    _lib.check(lib.pesto_rank_scores(h, S, offs.ctypes.data, C, side.ptr(yd), side.ptr(pd), side.ptr(counts), side.ptr(sc), side.kind, side.stream),
               lib.pesto_rank_last_error)
    return {"counts": side.result(counts), "scores": side.result(sc)}


def _score_row(row, y, p, offsets, model):
    v = scores(y, p, offsets, model)["scores"][:, row, :]
    return float(v[0, 0]) if offsets is None and v.shape[1] == 1 else v


def roc_auc(y, p, offsets=None, model=None):
    """metrics.roc_auc_score per column: float64 [S, C], or a float for one column"""
    return _score_row(0, y, p, offsets, model)


def pr_auc(y, p, offsets=None, model=None):
    """metrics.auc(recall, precision) of metrics.precision_recall_curve per column: float64 [S, C], or a float for one column"""
    return _score_row(1, y, p, offsets, model)


def f1(y, p, offsets=None, model=None):
    """metrics.f1_score(y, round(p)) per column: float64 [S, C], or a float for one column"""
    return _score_row(2, y, p, offsets, model)


def _curves(y, p, drop_intermediate, offsets, model, capacity=None):
    if capacity is not None and not 0 <= int(capacity) <= 2 ** 31 - 1:
        raise ValueError(f"capacity must be in 0 .. 2**31 - 1, got {capacity!r}")
    side, h, yd, pd, offs, S, C, single = _placed(y, p, offsets, model)
    cap = int(pd.shape[0]) * C if capacity is None else int(capacity)
    off = side.empty((S * C + 1,), np.int64)
    lib = _lib.load()
    for _ in range(2):
        thr, tps, fps = side.empty((cap,), np.float32), side.empty((cap,), np.int64), side.empty((cap,), np.int64)
        sz = np.zeros(1, np.int64)
        _lib.check(lib.pesto_rank_curves(h, S, offs.ctypes.data, C, side.ptr(yd), side.ptr(pd), int(bool(drop_intermediate)), cap, side.ptr(off),
                                         side.ptr(thr) if cap else None, side.ptr(tps) if cap else None, side.ptr(fps) if cap else None,
                                         sz.ctypes.data, side.kind, side.stream), lib.pesto_rank_last_error)
        K = int(sz[0])
        if K <= cap:
            return tuple(side.result(a) for a in (off, thr[:K], tps[:K], fps[:K])) + (single,)
        cap = K
    raise RuntimeError("the curve capacity did not converge")


def curves(y, p, drop_intermediate=False, offsets=None, model=None, capacity=None):
    """(offsets int64 [S C + 1], thr float32 [K], tps int64 [K], fps int64 [K]): column s * C + c owns the rows offsets[col]:offsets[col + 1],
    its distinct scores in descending order with the positives and negatives at or above each - sklearn's _binary_clf_curve. With
    drop_intermediate only the first point, the last point and the points where the second difference of fps or of tps is not zero remain
    (thinned on the device). capacity: the rows to allocate for the first attempt (default R * C, which always fits); the call is repeated
    once with the exact count if it was too small."""
    return _curves(y, p, drop_intermediate, offsets, model, capacity)[:4]


def _f64(a):
    return a.double() if _lib.is_torch(a) else a.astype(np.float64)


def _join(a, first=None, last=None):
    """a with a leading / trailing constant, as a's kind"""
    if _lib.is_torch(a):
        import torch
        parts = [a.new_full((1,), v) for v in ([] if first is None else [first])] + [a] + [a.new_full((1,), v) for v in ([] if last is None else [last])]
        return torch.cat(parts)
    return np.concatenate(([] if first is None else [first], a, [] if last is None else [last])).astype(a.dtype)


def _flip(a):
    return a.flip(0) if _lib.is_torch(a) else a[::-1].copy()


def _divide(a, b):
    """a / b in float64 (0 / 0 is NaN, without a warning)"""
    if _lib.is_torch(a):
        return a / b
    with np.errstate(invalid="ignore", divide="ignore"):
        return a / b


def roc_points(thr, tps, fps):
    """(fpr, tpr, thresholds) float64, float64, float32 of one column's integer curve, as metrics.roc_curve assembles them: the point
    (0, 0) with the threshold inf in front, fpr = fps / fps[-1], tpr = tps / tps[-1] (NaN without negatives / positives)."""
    t, f = _f64(_join(tps, first=0)), _f64(_join(fps, first=0))
    return _divide(f, f[-1]), _divide(t, t[-1]), _join(thr, first=np.inf)


def pr_points(thr, tps, fps):
    """(precision, recall, thresholds) of one column's integer curve, as metrics.precision_recall_curve assembles them: precision =
    tps / (tps + fps) (0 where the sum is 0), recall = tps / tps[-1] (1 without positives, as sklearn), in ascending threshold order with the
    closing point (precision 1, recall 0)."""
    t, s = _f64(tps), _f64(tps + fps)
    precision = _divide(t, s)
    precision[s == 0] = 0.0
    recall = _divide(t, t[-1]) if float(t[-1]) != 0 else t * 0.0 + 1.0
    return _join(_flip(precision), last=1.0), _join(_flip(recall), last=0.0), _flip(thr)


def _per_column(points, y, p, drop, offsets, model):
    off, thr, tps, fps, single = _curves(y, p, drop, offsets, model)
    o = _lib.host(off)
    out = [points(thr[o[c]:o[c + 1]], tps[o[c]:o[c + 1]], fps[o[c]:o[c + 1]]) for c in range(o.size - 1)]
    return out[0] if single else out


def roc_curve(y, p, drop_intermediate=True, offsets=None, model=None):
    """metrics.roc_curve(y, p, drop_intermediate=drop_intermediate): (fpr, tpr, thresholds), thresholds[0] = inf; a list of such triples,
    one per column, with offsets or several classes."""
    return _per_column(roc_points, y, p, drop_intermediate, offsets, model)


def precision_recall_curve(y, p, offsets=None, model=None):
    """metrics.precision_recall_curve(y, p): (precision, recall, thresholds), thresholds ascending, the last point (1, 0); a list of such
    triples, one per column, with offsets or several classes."""
    return _per_column(pr_points, y, p, False, offsets, model)


def auc(x, y):
    """metrics.auc(x, y): the trapezoid of y over x in float64 on the host; x must rise or fall monotonically (a falling x, such as the
    recall of precision_recall_curve, changes the sign)."""
    x, y = np.asarray(_lib.host(x), np.float64).reshape(-1), np.asarray(_lib.host(y), np.float64).reshape(-1)
    if x.size != y.size or x.size < 2:
        raise ValueError(f"x and y must have the same length of at least 2, got {x.size} and {y.size}")
    dx = np.diff(x)
    direction = 1.0
    if np.any(dx < 0):
        if not np.all(dx <= 0):
            raise ValueError("x is neither increasing nor decreasing")
        direction = -1.0
    return float(direction * (dx * (y[1:] + y[:-1]) / 2.0).sum())


def confidence_histogram(y, p, edges, offsets=None, model=None):
    """int64 [S, C, B, 2], or [B, 2] for one column: [..., v] = np.histogram(p[y == v], bins=edges) - B left-closed bins, the last one
    closed on both sides. edges: B + 1 float32 values rising strictly (other types are rounded to float32 first: the equality with
    np.histogram holds for float32 edges, which compare with the float32 scores as they are). The four histograms of interface_ppi_confidence.ipynb are slices."""
    e = np.asarray(_lib.host(edges)).reshape(-1)
    e32 = np.ascontiguousarray(e, np.float32)
    if e.size < 2 or np.any(np.isnan(e32)) or not np.all(e32[1:] > e32[:-1]):
        raise ValueError("edges must be at least 2 values rising strictly (as float32)")
    side, h, yd, pd, offs, S, C, single = _placed(y, p, offsets, model)
    B = e32.size - 1
    if S * C * B > 2 ** 31 - 1:
        raise ValueError(f"S * C * B must stay below 2**31, got {S} * {C} * {B}")
    counts = side.empty((S, C, B, 2), np.int64)
    lib = _lib.load()
    _lib.check(lib.pesto_rank_histogram(h, S, offs.ctypes.data, C, side.ptr(yd), side.ptr(pd), B, e32.ctypes.data, side.ptr(counts), side.kind,
                                        side.stream), lib.pesto_rank_last_error)
    counts = side.result(counts)
    return counts[0, 0] if single else counts
