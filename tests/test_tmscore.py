"""GPU tests of pesto_amd.tmscore (pesto_tmscore.hip) against the NumPy definition of test_tmscore_fixture.py, through host arrays and
ROCm tensors. The sweep systems keep a decision margin of 1e-7 A (asserted by the fixture), so the sets and with them counts, gdt_ts and
gdt_ha are compared by equality; tm within one float32 unit of float32(tm64) (with equal sets the two differ only by double rounding,
which can move one float32 rounding by at most a unit); seed by the definition's per-seed maxima within 1e-12; the fit by orthonormality
within 1e-12 and by the tm it reproduces in NumPy; rmsd by the bits of dockq.fit_rmsd. The sweep covers the lane word and its second
word (L of 63, 64, 65, 129, 257), the single-seed lengths (3, 4), F of 1, 2, 65; then the hand-worked cases, L = 4096, the ragged batch,
identical bits alone / in a batch / between the sides / from call to call, a rigid motion, a refused call and the recorded MD system.
The worst observed share of every bound is printed (pytest -s)."""
import numpy as np
import pytest

from conftest import golden
from test_docking_fixture import system, ulp_apart
from test_tmscore_fixture import BIG, MARGIN_CAP, SWEEP, d0_def, domain16, sweep_def, sweep_system, tm_def

pytestmark = pytest.mark.gpu

FIELDS = ("tm", "gdt_ts", "gdt_ha", "counts", "rmsd", "seed", "rotation", "translation")
DTYPES = dict(tm=np.float32, gdt_ts=np.float32, gdt_ha=np.float32, counts=np.int32, rmsd=np.float32, seed=np.int32, rotation=np.float64,
              translation=np.float64)
WORST = dict(tm_ulp=0, seed_gap=0.0, orthonormal=0.0, refit_ulp=0)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_result(a, b, rows=slice(None)):
    return all(same_bits(host(getattr(a, k)), host(getattr(b, k))[rows]) for k in FIELDS)


def check(out, want, ref, xyz, sel=None, scale=10.0, on_device=False, tag=""):
    """every assertion of the sweep on one result; ref [N, 3], xyz [F, N, 3] on the host"""
    from pesto_amd import dockq as Q
    F = xyz.shape[0]
    for k in FIELDS:
        v = getattr(out, k)
        assert (v.is_cuda if on_device else isinstance(v, np.ndarray)) and host(v).dtype == DTYPES[k], (tag, k)
    o = {k: host(getattr(out, k)) for k in FIELDS}
    assert o["counts"].shape == (F, 5) and o["rotation"].shape == (F, 3, 3) and o["translation"].shape == (F, 3)
    assert np.array_equal(o["counts"], want["counts"]), tag
    assert np.array_equal(o["gdt_ts"].view(np.uint32), want["gdt_ts"].view(np.uint32)), tag
    assert np.array_equal(o["gdt_ha"].view(np.uint32), want["gdt_ha"].view(np.uint32)), tag
    WORST["tm_ulp"] = max(WORST["tm_ulp"], ulp_apart(o["tm"], want["tm"]))
    assert ulp_apart(o["tm"], want["tm"]) <= 1, tag
    assert (o["seed"] >= 0).all() and (o["seed"] < want["per_seed"].shape[1]).all(), tag
    gap = float((want["tm64"] - want["per_seed"][np.arange(F), o["seed"]]).max())
    WORST["seed_gap"] = max(WORST["seed_gap"], gap)
    assert gap <= 1e-12, (tag, gap)
    R, t = o["rotation"], o["translation"]
    orth = float(np.abs(R @ R.transpose(0, 2, 1) - np.eye(3)).max())
    WORST["orthonormal"] = max(WORST["orthonormal"], orth, float(np.abs(np.linalg.det(R) - 1).max()))
    assert orth <= 1e-12 and np.abs(np.linalg.det(R) - 1).max() <= 1e-12, (tag, orth)
    idx = np.arange(ref.shape[0]) if sel is None else np.asarray(sel)
    X, Y = xyz[:, idx].astype(np.float64), ref[idx].astype(np.float64)
    L = idx.size
    D = np.sqrt(((X @ R + t[:, None] - Y[None]) ** 2).sum(-1)) * scale
    again = ((1.0 / (1.0 + (D / d0_def(L)) ** 2)).sum(1) / L).astype(np.float32)
    WORST["refit_ulp"] = max(WORST["refit_ulp"], ulp_apart(o["tm"], again))
    assert ulp_apart(o["tm"], again) <= 1, tag
    place = dev if on_device else (lambda a: a)
    assert same_bits(out.rmsd, Q.fit_rmsd(place(ref), place(xyz), idx, idx, scale)), tag
    print(f"{tag}: worst so far: tm {WORST['tm_ulp']} of 1 float32 unit, seed gap {WORST['seed_gap']:.3g} of 1e-12, "
          f"orthonormality {WORST['orthonormal']:.3g} of 1e-12, tm from the returned fit {WORST['refit_ulp']} of 1 float32 unit")


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "L%d-F%d-step%d" % c[:3])
def test_seeded_sweep(case, on_device):
    from pesto_amd import tmscore as T
    L, F, step, seed = case
    s, want = sweep_system(L, F, seed), sweep_def(*case)
    assert want["margin"] >= MARGIN_CAP
    place = dev if on_device else (lambda a: a)
    out = T.tm_score(place(s["ref"]), place(s["xyz"]), step=step)
    check(out, want, s["ref"], s["xyz"], on_device=on_device, tag=f"sweep L = {L}, F = {F}")


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_hand_worked_cases(on_device):
    from pesto_amd import tmscore as T
    place = dev if on_device else (lambda a: a)
    ref, x, w = domain16()
    out = T.tm_score(place(ref), place(ref[None]), scale=1.0)          # the reference itself: the identity, exactly 1
    assert host(out.tm)[0] == 1.0 and host(out.counts)[0].tolist() == [16] * 5 and host(out.seed)[0] == 0 and host(out.rmsd)[0] == 0.0
    assert host(out.gdt_ts)[0] == 1.0 and host(out.gdt_ha)[0] == 1.0
    assert np.array_equal(host(out.rotation)[0], np.eye(3)) and np.array_equal(host(out.translation)[0], np.zeros(3))
    out = T.tm_score(place(ref), place(x), scale=1.0)                   # the displaced domain: window (0, 8), fitted by the identity
    assert host(out.tm)[0] == np.float32((8 + 8 / 40001) / 16) and host(out.counts)[0].tolist() == [8] * 5 and host(out.seed)[0] == w
    assert host(out.gdt_ts)[0] == np.float32(0.5) and host(out.gdt_ha)[0] == np.float32(0.5)
    assert np.array_equal(host(out.rotation)[0], np.eye(3)) and np.array_equal(host(out.translation)[0], np.zeros(3))
    assert host(out.rmsd)[0] > 30                                       # the one global fit: far off
    g = T.gdt(place(ref), place(x), scale=1.0)
    assert same_bits(g.gdt_ts, out.gdt_ts) and same_bits(g.gdt_ha, out.gdt_ha) and same_bits(g.counts, out.counts)
    names = np.array(["N", "CA"] * 16)
    both = np.repeat(ref, 2, 0)
    both[::2] += np.float32(1.0)
    xb = np.repeat(x[0], 2, 0)[None]
    assert same_result(T.tm_ca(place(both), place(xb), names, scale=1.0), out)
    for L in (3, 4):                                                    # a single seed
        s = sweep_system(L, 2, 7)
        check(T.tm_score(place(s["ref"]), place(s["xyz"])), tm_def(s["ref"], s["xyz"]), s["ref"], s["xyz"], on_device=on_device, tag=f"L = {L}")
    s = sweep_system(5, 3, 1)                                           # a NaN frame between two finite ones
    xn = s["xyz"].copy()
    xn[1, 2, 1] = np.nan
    out, clean = T.tm_score(place(s["ref"]), place(xn)), T.tm_score(place(s["ref"]), place(s["xyz"]))
    for k in ("tm", "gdt_ts", "gdt_ha", "rmsd"):
        assert np.isnan(host(getattr(out, k))[1]), k
    assert host(out.seed)[1] == -1 and (host(out.counts)[1] == 0).all() and np.isnan(host(out.rotation)[1]).all() and np.isnan(host(out.translation)[1]).all()
    for k in FIELDS:
        assert same_bits(host(getattr(out, k))[[0, 2]], host(getattr(clean, k))[[0, 2]]), k
    with pytest.raises(ValueError, match="reference"):
        T.tm_score(place(xn[1]), place(s["xyz"]))


def test_norm_len_d0_and_iterations_follow_the_definition():
    from pesto_amd import tmscore as T
    s = sweep_system(63, 2, 0)
    sel = np.arange(3, 60)
    for kw in (dict(norm_len=80), dict(d0=2.5), dict(norm_len=80, d0=3.0), dict(n_iter=1), dict(n_iter=3, step=5)):
        want = tm_def(s["ref"], s["xyz"], sel, **kw)
        out = T.tm_score(s["ref"], s["xyz"], sel, **kw)
        assert want["margin"] >= MARGIN_CAP, kw
        assert np.array_equal(out.counts, want["counts"]) and ulp_apart(out.tm, want["tm"]) <= 1, kw
        assert np.array_equal(out.gdt_ts.view(np.uint32), want["gdt_ts"].view(np.uint32)), kw
        assert (want["tm64"] - want["per_seed"][np.arange(2), out.seed]).max() <= 1e-12, kw


def test_the_lds_and_register_limit():
    from pesto_amd import tmscore as T
    L, F, step, seed = BIG
    s, want = sweep_system(L, F, seed), sweep_def(*BIG)
    assert L == 4096 and want["margin"] >= MARGIN_CAP
    out = T.tm_score(dev(s["ref"]), dev(s["xyz"]), step=step)
    check(out, want, s["ref"], s["xyz"], on_device=True, tag="L = 4096")


def test_ragged_batch_against_single_calls():
    from pesto_amd import tmscore as T
    parts = [sweep_system(L, 1, 0) for L in (5, 64, 130)]
    pad = [np.zeros((2, 3), np.float32), np.full((1, 3), 9.0, np.float32), np.zeros((0, 3), np.float32)]      # atoms that sel leaves out
    ref = np.concatenate([a for p, e in zip(parts, pad) for a in (p["ref"], e)])
    xyz = np.concatenate([a for p, e in zip(parts, pad) for a in (p["xyz"][0], e + 1)])[None]
    sizes = [7, 65, 130]
    sel = np.concatenate([np.arange(5), 7 + np.arange(64), 72 + np.arange(130)])
    for place in (lambda a: a, dev):
        out = T.tm_score(place(ref), place(xyz), sel, sizes=sizes)
        assert host(out.tm).shape == (3,) and host(out.rotation).shape == (3, 3, 3)
        for b, p in enumerate(parts):
            assert same_result(T.tm_score(place(p["ref"]), place(p["xyz"])), out, slice(b, b + 1)), b
        two = T.tm_score(place(ref), place(xyz), sel, sizes=sizes, norm_len=[5, 100, 130], d0=[0.5, 3.0, 4.0])
        assert same_result(T.tm_score(place(parts[1]["ref"]), place(parts[1]["xyz"]), norm_len=100, d0=3.0), two, slice(1, 2))


def test_identical_bits_alone_in_a_batch_between_sides_and_calls():
    from pesto_amd import tmscore as T
    s = sweep_system(64, 65, 2)
    batch = T.tm_score(s["ref"], s["xyz"])
    assert same_result(T.tm_score(s["ref"], s["xyz"]), batch)                                       # a second call
    assert same_result(T.tm_score(dev(s["ref"]), dev(s["xyz"])), batch)                             # the other side
    for f in (0, 37, 64):
        assert same_result(T.tm_score(s["ref"], s["xyz"][f:f + 1]), batch, slice(f, f + 1)), f       # alone: other shares of the seeds
        assert same_result(T.tm_score(dev(s["ref"]), dev(s["xyz"][f:f + 1])), batch, slice(f, f + 1)), f


def test_a_rigid_motion_of_the_whole_model_scores_one():
    from pesto_amd import tmscore as T
    ref = np.round(sweep_system(65, 1, 0)["ref"].astype(np.float64) * 1024) / 1024                  # dyadic: the motion below is exact
    x = (ref[:, [1, 2, 0]] * np.array([1.0, -1.0, -1.0]) + np.array([0.25, -1.5, 2.0]))             # a proper signed axis permutation, a shift
    ref32, x32 = ref.astype(np.float32), x.astype(np.float32)
    assert np.array_equal(ref32, ref) and np.array_equal(x32, x)
    out = T.tm_score(ref32, x32[None])
    below = np.nextafter(np.float32(1), np.float32(0))
    assert out.tm[0] in (np.float32(1), below) and out.counts[0].tolist() == [65] * 5 and out.gdt_ha[0] == 1.0
    X = x @ out.rotation[0] + out.translation[0]
    d = np.sqrt(((X - ref) ** 2).sum(1)) * 10.0
    tm64 = (1.0 / (1.0 + (d / d0_def(65)) ** 2)).sum() / 65
    print(f"rigid motion: 1 - tm = {1 - tm64:.3g} of 1e-12, largest distance {d.max():.3g} A")
    assert tm64 >= 1 - 1e-12 and out.rmsd[0] < 1e-5


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_refused_call_writes_nothing(on_device):
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    s = sweep_system(5, 3, 1)
    F, N = s["xyz"].shape[:2]
    model, lib = _default_model(0), _lib.load()
    place = dev if on_device else (lambda a: np.ascontiguousarray(a))
    side = _lib.Side(place(s["xyz"]), model._gpu)
    kinds = ((np.float32, 1), (np.float32, 1), (np.float32, 1), (np.int32, 5), (np.float32, 1), (np.int32, 1), (np.float64, 9), (np.float64, 3))
    so, ln, dz = np.array([0, N], np.int32), np.array([float(N)]), np.array([0.5])

    def call(sel, **kw):
        sd, x, y = place(np.asarray(sel, np.int32)), place(s["xyz"]), place(s["ref"])
        outs = [place(np.full(F * w, 7, dt)) for dt, w in kinds]
        a = dict(so=so, step=1, n_iter=20, scale=10.0)
        a.update(kw)
        rc = lib.pesto_tmscore(model.handle, F, N, 1, a["so"].ctypes.data, side.ptr(sd), side.ptr(y), side.ptr(x), ln.ctypes.data, dz.ctypes.data, a["step"],
                               a["n_iter"], a["scale"], *(side.ptr(o) for o in outs), side.kind, side.stream)
        return rc, [host(o) for o in outs]

    rc, good = call(np.arange(N))
    assert rc == 0 and all(not (o == 7).any() for o in good[:3])
    for sel in ([0, 1, 2, 3, N], [-1, 1, 2, 3, 4], [0, 1, 2 ** 30, 3, 4]):
        rc, outs = call(sel)
        assert rc == -1 and b"[0, N)" in lib.pesto_tmscore_last_error(), sel
        assert all((o == 7).all() for o in outs), sel
    for kw in (dict(step=0), dict(n_iter=0), dict(scale=0.0), dict(so=np.array([0, 2], np.int32)), dict(so=np.array([1, N], np.int32))):
        rc, outs = call(np.arange(N), **kw)                             # what the host refuses before any launch
        assert rc == -1 and all((o == 7).all() for o in outs), kw
    rc, again = call(np.arange(N))                                      # the next call is served
    assert rc == 0 and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(again, good))


def test_recorded_md_system():
    from pesto_amd import tmscore as T
    s = system(golden("docking"), "iface")
    ca = np.nonzero(s["ca"])[0]
    want = tm_def(s["xyz"][0], s["xyz"], ca, step=8)          # (recorded inputs: steps 1, 2, 3 and 6 meet a 7.6e-8 A margin, below the cap)
    print(f"recorded MD system: {s['xyz'].shape[0]} frames, {ca.size} CA atoms, decision margin {want['margin']:.3g} A, "
          f"tm {want['tm64'].min():.4f} .. {want['tm64'].max():.4f}")
    assert want["margin"] >= MARGIN_CAP                                 # (recorded inputs: the same condition as on the sweep's)
    for place, on_device in ((lambda a: a, False), (dev, True)):
        out = T.tm_score(place(s["xyz"][0]), place(s["xyz"]), ca, step=8)
        check(out, want, s["xyz"][0], s["xyz"], sel=ca, on_device=on_device, tag="recorded MD system")
        assert host(out.tm)[0] == 1.0 and host(out.rmsd)[0] == 0.0


def test_structure_tmscore_matches_atoms_as_structure_lddt_does():
    from pesto_amd import lddt as Ld
    from pesto_amd import tmscore as T
    from test_lddt_fixture import perturbed_1thf
    ref, model, gone, _ = perturbed_1thf()
    y, x, res, chain, table = Ld.match_atoms(ref, model)
    names = np.asarray(Ld._structure_dict(ref)["name"]).astype(str)
    ca = names == "CA"
    sel = np.nonzero(ca & np.isfinite(x[0]).all(1))[0]
    out, tab = T.structure_tmscore(ref, model)
    assert tab["n_ref"] == int(ca.sum()) == sel.size + 1 and tab["resid"].size == sel.size
    assert not ((tab["chain_name"] == gone[0]) & (tab["resid"] == gone[1])).any()
    assert same_result(out, T.tm_score(y, x, sel, norm_len=int(ca.sum()), scale=1.0))
    assert 0.9 < out.tm[0] < 1 and out.gdt_ts[0] > 0.8
