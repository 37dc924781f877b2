"""GPU sweeps over the seeded cases of tests/assembly_sweep.py (generators and definitions checked without a GPU by
tests/test_assembly_sweep_fixture.py): everything of pesto_contacts behind the cell-grid search - the regroup radix sort, the one-workgroup
scans, the typed keys, the swapped keys' second sort, the capacity protocol -, k_bc_scores, both paths of pesto_interface_patches and
k_contact_labels with multi-bit masks and a receptor subset, at the tile edges of the kernels' constants.

What is exact: pairs, d, all four group columns, keys, reverse keys, T, tie flags, K, G, U; score rows 0 to 6 (the counts are integers,
float32 division and square root are correctly rounded, 2U is an integer and auc one float64 division of exact operands); patch_of,
n_patches, patch_size and patch_mean on both paths and on repeats; labels and label ties. What has a tolerance: the std row, one float32
spacing about the float32 of the float64 unbiased std (the float64 accumulation error, about R 2^-52, is far below 2^-24).

Every case runs from ROCm tensors; every third case of a list from host arrays too, with identical bytes."""
import time

import numpy as np
import pytest

import assembly_sweep as S
from test_analysis_sweep import close, dev, exact, host, place, same_bytes  # noqa: F401

pytestmark = pytest.mark.gpu


def sides(entry, case):
    return [True, False] if S.every_third(entry, case) else [True]


@pytest.fixture(scope="module")
def model():
    import torch
    from pesto_amd.patches import _default_model
    assert torch.cuda.is_available()
    return _default_model(0)                 # a weightless handle: nothing here runs the forward


# ================================================================== pesto_contacts
CONTACT_KEYS = ("pairs", "d", "groups", "keys", "rkeys", "T", "ties")


def contacts_with_capacities(model, c, cap, capg, on_device):
    """pesto_contacts with the given capacities, marshalled as dataset._contacts_call does -> (sizes, arrays whole, up to their capacity)"""
    from pesto_amd import _lib
    n, nt = c["X"].shape[0], c["n_types"]
    offs = _lib.offsets([int(v) for v in c["sizes"]])
    (X,) = place(on_device, c["X"])
    side = _lib.Side(X, model._gpu)
    Xs, sub = side.put(X, np.float32, (n, 3), "X"), side.put(c["sub"], np.int32, (n,), "subunit")
    res, typ = side.put(c["res"], np.int32, (n,), "residue"), side.put(c["typ"], np.int32, (n,), "type")
    out = dict(pairs=side.empty((cap, 2), np.int32), d=side.empty((cap,), np.float32), groups=side.empty((capg, 4), np.int32),
               keys=side.empty((cap, 4), np.int16), rkeys=side.empty((cap, 4), np.int16), T=side.empty((capg, nt, nt), np.uint8),
               ties=side.empty((n,), np.uint8))
    sz = np.zeros(3, np.int64)
    lib = _lib.load()
    _lib.check(lib.pesto_contacts(model.handle, n, len(offs) - 1, offs.ctypes.data, c["n_sub"], side.ptr(Xs), side.ptr(sub), side.ptr(res), side.ptr(typ),
                                  nt, S.R_THR, cap, capg, *(side.ptr(out[k]) for k in CONTACT_KEYS), sz.ctypes.data, side.kind, side.stream),
               lib.pesto_contacts_last_error)
    return tuple(int(v) for v in sz), out


def check_contacts(case, tag, out, w):
    """out: arrays sliced to their sizes"""
    for k in CONTACT_KEYS:
        exact(case, f"{tag}{k}", out[k], w[k])


@pytest.mark.parametrize("case", S.CONTACTS[:-1], ids=S.ident)
def test_contacts_regroup_typed_keys_and_capacities(case, model):
    from pesto_amd import dataset
    t0 = time.perf_counter()
    c = S.build("contacts", case)
    w = c["want"]
    K, G, U = w["K"], w["G"], w["U"]
    runs = []
    for on_device in sides("contacts", case):
        out, _ = dataset._contacts_call(model, c["rows"], S.R_THR, list(range(c["n_types"])), on_device)
        assert (out["K"], out["G"], out["U"]) == (K, G, U), (case, (out["K"], out["G"], out["U"]), (K, G, U))
        got = {k: host(out[k]) for k in CONTACT_KEYS}
        check_contacts(case, "", got, w)
        # capacities exactly K and G
        sz, full = contacts_with_capacities(model, c, max(K, 1), max(G, 1), on_device)
        assert sz == (K, G, U), (case, "exact capacities", sz, (K, G, U))
        check_contacts(case, "exact capacities: ", {k: host(full[k])[:n] for k, n in zip(CONTACT_KEYS, (K, K, G, U, U, G, None))}, w)
        if K >= 2:                             # one pair short: the count comes back, nothing else, and no error
            sz, _ = contacts_with_capacities(model, c, K - 1, max(G, 1), on_device)
            assert sz == (K, -1, -1), (case, "cap_pairs = K - 1", sz)
        if G >= 2:                             # one group short: all three sizes
            sz, short = contacts_with_capacities(model, c, K, G - 1, on_device)
            assert sz == (K, G, U), (case, "cap_groups = G - 1", sz, (K, G, U))
            exact(case, "cap_groups = G - 1: ties", short["ties"], w["ties"])
        runs.append(got)
    if len(runs) == 2:
        same_bytes(case, *runs)
    print(f"{S.ident(case)}: K {K} G {G} U {U}, {time.perf_counter() - t0:.2f} s")


def test_contacts_big_ball_takes_three_calls(model, monkeypatch):
    """260 subunits of two atoms in one ball: K = 134,680 and G = 33,670 (group bit 14 is key bit 56, the last radix pass); the default
    capacities of _contacts_call hold neither, so the call repeats twice"""
    from pesto_amd import _lib, dataset
    case = S.BIG_BALL
    c = S.build("contacts", case)
    w = c["want"]
    assert (w["K"], w["G"]) == (134680, 33670)
    lib = _lib.load()
    calls = []

    class Counting:
        def __getattr__(self, name):
            f = getattr(lib, name)
            if name != "pesto_contacts":
                return f

            def counted(*a):
                calls.append(1)
                return f(*a)
            return counted
    monkeypatch.setattr(_lib, "load", lambda: Counting())
    out, _ = dataset._contacts_call(model, c["rows"], S.R_THR, list(range(c["n_types"])), True)
    assert len(calls) == 3, len(calls)
    assert (out["K"], out["G"], out["U"]) == (w["K"], w["G"], w["U"])
    check_contacts(case, "", {k: host(out[k]) for k in CONTACT_KEYS}, w)


# ================================================================== k_bc_scores
@pytest.mark.parametrize("case", S.SCORES, ids=S.ident)
def test_bc_scores(case, model):
    from pesto_amd.evaluate import bc_scores_batch
    t0 = time.perf_counter()
    c = S.build("scores", case)
    want = c["want"]
    runs = []
    for on_device in sides("scores", case):
        ys, ps = [place(on_device, *l) for l in (c["ys"], c["ps"])]
        got = host(bc_scores_batch(model, ys, ps))
        assert got.dtype == np.float32 and got.shape == want.shape, (case, got.dtype, got.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (case, "NaN pattern", np.argwhere(np.isnan(got) != np.isnan(want))[:5].tolist())
        clean = lambda a: np.where(np.isnan(a), np.float32(0), a)           # noqa: E731  (the NaN pattern is compared above, not the payloads)
        for row, name in enumerate(("acc", "ppv", "npv", "tpr", "tnr", "mcc", "auc")):
            exact(case, name, clean(got[:, row]), clean(want[:, row]))
        g, w = clean(got[:, 7]).astype(np.float64), clean(want[:, 7]).astype(np.float64)
        spacing = np.spacing(np.abs(clean(want[:, 7]))).astype(np.float64)
        off = np.abs(g - w) / spacing
        worst = float(off.max())
        print(f"{S.ident(case)} std: {int((off != 0).sum())} of {off.size} differ at all, worst {worst:.2f} float32 spacings")
        close(case, "std", np.where(np.isnan(want[:, 7]), np.nan, g), np.where(np.isnan(want[:, 7]), np.nan, w), float(spacing.max()))
        assert worst <= 1.0, (case, "std off by more than one float32 spacing", worst, np.unravel_index(int(np.argmax(off)), off.shape))
        runs.append(dict(scores=got))
    if len(runs) == 2:
        same_bytes(case, *runs)
    print(f"{S.ident(case)}: {time.perf_counter() - t0:.2f} s")


# ================================================================== pesto_interface_patches, both paths
@pytest.mark.parametrize("case", S.PATCHES, ids=S.ident)
def test_patches_both_paths(case, model):
    from pesto_amd.patches import interface_patches_batch, patch_labels
    t0 = time.perf_counter()
    c = S.build("patches", case)
    names = ("patch_of", "n_patches", "patch_size", "patch_mean")
    runs = []
    for on_device in sides("patches", case):
        ps, xs, afss, hs = [place(on_device, *l) for l in (c["ps"], c["xyzs"], c["afss"], c["has"])]
        out = {}
        for force_large in (False, True):
            for repeat in (0, 1):
                got = patch_labels(model, ps, xs, afss, hs, sel=c["sels"], afs_thr=S.THR[0], p_thr=S.THR[1], d_thr=S.THR[2], force_large=force_large)
                for name, g in zip(names, got[:4]):
                    tag = f"{name} ({'large' if force_large else 'default'} path, call {repeat})"
                    exact(case, tag, g, c[name])
                    out[tag] = host(g)
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)
    if len(c["sels"]) == 15:                   # the lists of the batch entry point: members ascending, patches in the order of their smallest row
        lists = interface_patches_batch(model, c["ps"], c["xyzs"], c["afss"], c["has"], afs_thr=S.THR[0], p_thr=S.THR[1], d_thr=S.THR[2])
        o = 0
        for s, per in enumerate(lists):
            R = c["ps"][s].shape[0]
            for k, members in enumerate(per.values()):
                lab = c["patch_of"][k, o:o + R]
                assert members == [np.nonzero(lab == q)[0].tolist() for q in range(c["n_patches"][s, k])], (case, s, k)
            o += R
    print(f"{S.ident(case)}: {time.perf_counter() - t0:.2f} s")


# ================================================================== k_contact_labels
@pytest.mark.parametrize("case", S.LABELS, ids=S.ident)
def test_contact_labels_masks_and_receptors(case, model):
    from pesto_amd import evaluate
    c = S.build("labels", case)
    runs = []
    for on_device in [True, False]:
        (X,) = place(on_device, c["X"])
        labels, ties = evaluate.contact_labels(model, X, c["sub"], c["res"], c["receptor"], c["mask"], [int(v) for v in c["sizes"]], c["n_res"], S.R_THR)
        out = dict(labels=host(labels), ties=host(ties))
        exact(case, "labels", out["labels"], c["labels"])
        exact(case, "ties", out["ties"], c["ties"])
        runs.append(out)
    same_bytes(case, *runs)
