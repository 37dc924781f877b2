"""GPU tests of pesto_amd.poses (pesto_poses.hip) against the NumPy definitions of test_poses_fixture.py, through host arrays and ROCm
tensors: the seeded sweep of pose_scores at the edges of the wave (64), the workgroup (256) and the mask word (32) - counts and masks
exactly, the double sums within the standard bound of a sum of n terms, the score within one float32 unit; docking.frame_contacts and
frame_residue_contacts on the materialised frames as a second yardstick; special inputs; materialize bit for bit; slide_to_contact bit
for bit and the contact it promises, within a bound derived here; top_poses; guided_dock against the composition of its pieces;
identical bits from call to call, between the two sides and for a pose alone; and refused calls, which write nothing."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_docking_fixture import dist_def, ulp_apart
from test_poses_fixture import (SWEEP, TINY, TINY_SCORE, place_def, scores_def, slide_def, sweep_args, sweep_definition, sweep_slide, sweep_system,
                                tiny, tiny_args, tiny_slides, top_def)

pytestmark = pytest.mark.gpu

COUNTS = ("n_contact", "n_clash", "n_res_R", "n_res_L", "n_pairs")
SUMS = ("w_R", "w_L", "w_pair")
U64 = 2.0 ** -53
BIG = (257, 255, 256, 33, 31)           # the sweep's largest case, which the other tests draw too


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int32) if a.dtype == np.uint32 else a).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype.itemsize == b.dtype.itemsize and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_scores(a, b):
    return all((x is None and y is None) or same_bits(x, y) for x, y in zip(a, b))


def check_against_definition(out, want, on_device, tag):
    """the asserts of the sweep on one result; returns the worst share of the double sums' bound"""
    F = want["n_contact"].shape[0]
    for key, dt in [(k, np.int32) for k in COUNTS] + [(k, np.float64) for k in SUMS] + [("score", np.float32)]:
        v = getattr(out, key)
        assert (v.is_cuda if on_device else isinstance(v, np.ndarray)) and host(v).dtype == dt and host(v).shape == (F,), key
    for key in COUNTS:
        assert np.array_equal(host(getattr(out, key)), want[key]), (tag, key)
    assert np.array_equal(host(out.masks).view(np.uint32), want["masks"]), tag
    worst = 0.0
    for key in SUMS:                                    # a double sum of n terms: within n 2^-53 sum|terms| of its exact value
        got, ref = host(getattr(out, key)), want[key]
        tol = want["n_" + key] * U64 * ref              # (every term is >= 0: the sum is its own sum of absolute values)
        err = np.abs(got - ref)
        assert (err <= tol).all(), (tag, key, float(err.max()))
        worst = max(worst, float((err[tol > 0] / tol[tol > 0]).max()) if (tol > 0).any() else 0.0)
    assert ulp_apart(host(out.score), want["score"]) <= 1, tag
    print(f"{tag}: worst share of the double sums' bound {worst:.3f}")
    return worst


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "F%d-NR%d-NL%d-RR%d-RL%d" % c)
def test_seeded_sweep(case, on_device):
    from pesto_amd import poses as P
    s, want = sweep_system(*case), sweep_definition(*case)
    args = [dev(v) if on_device else v for v in sweep_args(s)]
    out = P.pose_scores(*args, masks=True)
    check_against_definition(out, want, on_device, "F%d-NR%d-NL%d-RR%d-RL%d" % case)
    assert P.pose_scores(*args).masks is None
    if case[0] >= 65:                                   # the pose 100 nm away: all zeros, score 0
        assert [int(host(getattr(out, k))[-2]) for k in COUNTS] == [0] * 5 and host(out.score)[-2] == 0 and not host(out.masks)[-2].any()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_hand_worked_case(on_device):
    from pesto_amd import poses as P
    c = tiny()
    args = [dev(v) if on_device else v for v in tiny_args(c)]
    out = P.pose_scores(*args, r_contact=5.0, r_clash=3.0, scale=1.0, masks=True)
    for k, v in TINY.items():
        assert host(getattr(out, k)).tolist() == v, k                      # the double sums are exact here
    assert ulp_apart(host(out.score), np.array(TINY_SCORE, np.float32)) <= 1 and host(out.score)[3] == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_existing_kernels_agree_on_the_materialised_frames(on_device):
    """docking.frame_contacts gives the same n_contact from its offsets and frame_residue_contacts the same n_pairs"""
    from pesto_amd import docking as D
    from pesto_amd import poses as P
    case = (65, 64, 255, 32, 33)
    s, want = sweep_system(*case), sweep_definition(*case)
    xR, xL, rot, tr = (dev(s[k]) if on_device else s[k] for k in ("xyz_R", "xyz_L", "rotations", "translations"))
    frames = P.materialize(xL, rot, tr, xyz_R=xR)
    assert (frames.is_cuda if on_device else isinstance(frames, np.ndarray)) and tuple(frames.shape) == (65, 64 + 255, 3)
    a, b = frames[:, :64], frames[:, 64:]
    off, pairs, d = D.frame_contacts(a, b)
    assert np.array_equal(np.diff(host(off)), want["n_contact"])
    roff, _, _ = D.frame_residue_contacts((off, pairs, d), None, s["res_R"], s["res_L"])
    assert np.array_equal(np.diff(host(roff)), want["n_pairs"])
    out = P.pose_scores(xR, xL, s["res_R"], s["res_L"], rot, tr, s["p_R"], s["p_L"])
    assert np.array_equal(host(out.n_contact), np.diff(host(off))) and np.array_equal(host(out.n_pairs), np.diff(host(roff)))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_materialize_is_the_placement_bit_for_bit(on_device):
    from pesto_amd import poses as P
    for case in ((2, 63, 64, 31, 32), BIG):
        s = sweep_system(*case)
        want = place_def(s["xyz_L"], s["rotations"], s["translations"])
        xR, xL, rot, tr = (dev(s[k]) if on_device else s[k] for k in ("xyz_R", "xyz_L", "rotations", "translations"))
        y = P.materialize(xL, rot, tr)
        assert (y.is_cuda if on_device else isinstance(y, np.ndarray)) and same_bits(y, want)
        both = host(P.materialize(xL, rot, tr, xyz_R=xR))
        assert same_bits(both[:, case[1]:], want) and all(same_bits(f[:case[1]], s["xyz_R"]) for f in both)
    # a matrix that is no rotation is applied as it is
    R = np.array([[[2, 0.5, 0], [0, -1, 3], [0.25, 0, 0]]], np.float32)
    t = np.array([[1, 2, 3]], np.float32)
    assert same_bits(P.materialize(s["xyz_L"], R, t), place_def(s["xyz_L"], R, t))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_special_inputs(on_device):
    from pesto_amd import poses as P
    put = (lambda v: dev(v)) if on_device else (lambda v: v)
    case = (65, 256, 63, 65, 1)
    s = sweep_system(*case)
    base = dict(zip(("xyz_R", "xyz_L", "res_R", "res_L", "rotations", "translations", "p_R", "p_L"), sweep_args(s)))

    def run(**kw):
        a = dict(base, **kw)
        order = ("xyz_R", "xyz_L", "res_R", "res_L", "rotations", "translations", "p_R", "p_L")
        out = P.pose_scores(*(put(a[k]) for k in order), masks=True)
        return out, scores_def(*(a[k] for k in order))

    # a NaN ligand coordinate: that atom is in no pair
    xL = s["xyz_L"].copy()
    xL[7, 1] = np.nan
    out, want = run(xyz_L=xL)
    check_against_definition(out, want, on_device, "NaN ligand atom")
    lost = sweep_definition(*case)["n_contact"] - want["n_contact"]
    assert (lost >= 0).all() and lost.max() > 0
    # a non-finite receptor coordinate: that atom is in no pair (the grid is built on a copy without it), the same definition
    for bad in (np.nan, np.inf, -np.inf):
        xR = s["xyz_R"].copy()
        xR[100, 2] = bad
        out, want = run(xyz_R=xR)
        check_against_definition(out, want, on_device, f"receptor atom at {bad}")
        assert want["n_contact"].max() > 100
    # receptors whose atoms are all NaN on one axis, on every axis, and the one-atom receptor with a NaN: nothing is a contact, and the
    # grid's box must not be taken from them
    for label, xR in (("NaN axis", np.where(np.arange(3) == 1, np.nan, s["xyz_R"])), ("all NaN", np.full_like(s["xyz_R"], np.nan)),
                      ("all but atom 5 non-finite", np.where((np.arange(256) == 5)[:, None], s["xyz_R"], np.float32(np.inf)))):
        out, want = run(xyz_R=xR.astype(np.float32))
        check_against_definition(out, want, on_device, label)
        assert label == "all but atom 5 non-finite" or not want["n_contact"].any()
    assert want["n_contact"].max() > 0 and want["n_res_R"].max() == 1                   # (atom 5 alone is still met)
    for one in ([np.nan, 0.5, 0.5], [3.0, np.nan, np.nan], [np.nan] * 3, [np.inf, -2.0, 1.0]):
        out, want = run(xyz_R=np.array([one], np.float32), res_R=np.zeros(1, np.int32), p_R=s["p_R"][:1])
        check_against_definition(out, want, on_device, f"one-atom receptor at {one}")
        assert not want["n_contact"].any() and not host(out.score).any() and not host(out.masks).any()
    # a one-atom receptor, against a ligand of one residue
    out, want = run(xyz_R=s["xyz_R"][:1], res_R=np.zeros(1, np.int32), p_R=s["p_R"][:1])
    check_against_definition(out, want, on_device, "one-atom receptor")
    assert want["n_contact"].max() > 0 and want["n_res_R"].max() == 1
    # r_contact = r_clash = 0: nothing is a contact; a threshold that holds everything: every pair is one
    a = [put(v) for v in sweep_args(s)]
    none = P.pose_scores(*a, r_contact=0.0, r_clash=0.0)
    assert not host(none.n_contact).any() and not host(none.score).any()
    every = P.pose_scores(*(put(v) for v in (s["xyz_R"], s["xyz_L"], s["res_R"], s["res_L"], s["rotations"][:8], s["translations"][:8], s["p_R"], s["p_L"])),
                          r_contact=1e4, r_clash=1e4)
    assert (host(every.n_contact) == 256 * 63).all() and (host(every.n_clash) == 256 * 63).all() and (host(every.n_pairs) == 65).all()
    # the identity pose of a complex: a pose's own frame as the ligand, placed by (I, 0), gives that pose's bits
    k = int(np.argmax(sweep_definition(*case)["n_contact"]))
    bound = host(P.materialize(put(s["xyz_L"]), put(s["rotations"][k:k + 1]), put(s["translations"][k:k + 1])))[0]
    one = P.pose_scores(put(s["xyz_R"]), put(bound), s["res_R"], s["res_L"], np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32),
                        s["p_R"], s["p_L"], masks=True)
    ref = P.pose_scores(*a, masks=True)
    assert all(same_bits(x, y[k:k + 1]) for x, y in zip(one, ref)) and host(one.n_contact)[0] > 100


def slide_bound(s, sl, t, r_touch, scale):
    """per pose, in the distance's unit: how far min d over the materialised pose may lie from r_touch. With q = fl(R x) the placement
    gives y' = (q + t)(1 + d1) at the slid pose and y = (q + o)(1 + d2) at the origin, |d| <= 2^-24, and t = (o + s u)(1 + d3); so a
    placed atom lies within e = 2^-24 (|t| + |y'| + |y|) per component, sqrt(3) e in length, of the point y + s u the definition
    speaks of. There the touching pair is at sqrt(rho^2 + s^2 eps) and no pair is nearer than sqrt(rho^2 - s^2 |eps|), eps = |u|^2 - 1
    of the float32 direction: within s^2 |eps| / rho of rho. The float32 distance itself carries 5 units of 2^-24 (three differences,
    the sum of squares halved by the root, the root, the scale). The double arithmetic of s is far below all of these."""
    o, u = s["translations"].astype(np.float64), s["directions"].astype(np.float64)
    y0 = np.abs(place_def(s["xyz_L"], s["rotations"], s["translations"]).astype(np.float64)).max(1)
    with np.errstate(invalid="ignore"):
        y1 = np.abs(place_def(s["xyz_L"], s["rotations"], t).astype(np.float64)).max(1)
    e = 2.0 ** -24 * (np.abs(t.astype(np.float64)) + y1 + y0).max(1)
    eps = np.abs((u * u).sum(1) - 1.0)
    rho = float(np.float32(r_touch)) / float(np.float32(scale))
    return scale * (np.sqrt(3.0) * e + sl * sl * eps / rho) + 5 * 2.0 ** -24 * r_touch


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", [(2, 63, 64, 31, 32), (65, 64, 255, 32, 33), BIG, (65, 257, 65, 1, 33)], ids=lambda c: "F%d-NR%d-NL%d" % c[:3])
def test_slide_to_contact(case, on_device):
    from pesto_amd import poses as P
    s = sweep_system(*case)
    want_s, want_t, want_pair = sweep_slide(*case)
    keys = ("xyz_R", "xyz_L", "rotations", "translations", "directions")
    sl, t, pair = P.slide_to_contact(*(dev(s[k]) if on_device else s[k] for k in keys))
    assert (sl.is_cuda if on_device else isinstance(sl, np.ndarray)) and host(sl).dtype == np.float64 and host(pair).dtype == np.int32
    assert same_bits(sl, want_s) and same_bits(t, want_t) and np.array_equal(host(pair), want_pair)        # (NaN rows included)
    hit = ~np.isnan(want_s)
    if not hit.any():
        return
    # after the slide the ligand touches: min d over the materialised pose is r_touch within the bound, and nothing clashes just below
    r_touch, scale = 3.5, 10.0
    rot_h, t_h = s["rotations"][hit], host(t)[hit]
    y = host(P.materialize(s["xyz_L"], rot_h, t_h))
    dmin = dist_def(np.repeat(s["xyz_R"][None], y.shape[0], 0), y, scale).min((1, 2)).astype(np.float64)
    tol = slide_bound(dict(s, rotations=rot_h, translations=s["translations"][hit], directions=s["directions"][hit]), want_s[hit], t_h, r_touch, scale)
    err = np.abs(dmin - r_touch)
    print(f"F{case[0]}: min d - r_touch up to {err.max():.3e}, bound {tol[np.argmax(err / tol)]:.3e}, worst share {(err / tol).max():.3f}")
    assert (err <= tol).all()
    r_clash = float(np.nextafter(np.float32(r_touch - tol.max()), np.float32(-np.inf)))
    out = P.pose_scores(s["xyz_R"], s["xyz_L"], s["res_R"], s["res_L"], rot_h, t_h, s["p_R"], s["p_L"], r_contact=5.0, r_clash=r_clash)
    assert not host(out.n_clash).any() and (host(out.n_contact) > 0).all()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_hand_worked_slides(on_device):
    from pesto_amd import poses as P
    eye, o, u = np.eye(3, dtype=np.float32)[None], np.zeros((1, 3), np.float32), np.array([[1, 0, 0]], np.float32)
    for xR, xL, want, want_pair in tiny_slides():
        sl, t, pair = P.slide_to_contact(*(dev(v) if on_device else v for v in (xR, xL, eye, o, u)), r_touch=2.0, scale=1.0)
        assert host(pair).tolist() == [want_pair]
        assert same_bits(sl, np.array([want])) and same_bits(t, np.array([[want, 0 if want == want else want, 0 if want == want else want]], np.float32))


def radix_tile():
    src = open(os.path.join(ROOT, "pesto_amd", "csrc", "pesto_radix.h")).read()
    return int(re.search(r"RADIX_NT = (\d+)", src).group(1)) * int(re.search(r"RADIX_ITEMS = (\d+)", src).group(1))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_top_poses(on_device):
    from pesto_amd import poses as P
    tile = radix_tile()
    assert tile >= 256
    rng = np.random.default_rng(5)
    values = np.array([0.0, -0.0, 0.25, 0.5, 0.5000001, 1.0, -1.0, np.inf, -np.inf, np.nan, 1e-40, -1e-40], np.float32)
    for F in (1, 255, 256, 257, tile + 1, 2 * tile + 3):
        score = np.where(rng.random(F) < 0.5, rng.choice(values, F), rng.random(F).astype(np.float32)).astype(np.float32)
        clash = rng.integers(0, 4, F).astype(np.int32)
        sd, cd = (dev(score), dev(clash)) if on_device else (score, clash)
        for k, kw in ((F + 5, {}), (F, dict(n_clash=cd)), (max(F // 3, 1), dict(n_clash=cd, max_clash=2)), (0, {}), (7, dict(n_clash=cd, max_clash=-1))):
            got = P.top_poses(sd, k, **kw)
            ref = top_def(score, k, clash if kw else None, kw.get("max_clash", 0))
            assert (got.is_cuda if on_device else isinstance(got, np.ndarray)) and host(got).dtype == np.int32
            assert np.array_equal(host(got), ref), (F, k, kw)
    assert host(P.top_poses(np.full(3, np.nan, np.float32), 3)).size == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_guided_dock_is_the_composition_of_its_pieces(on_device):
    from pesto_amd import poses as P
    s = sweep_system(*BIG)
    xR, xL = (dev(s[k]) if on_device else s[k] for k in ("xyz_R", "xyz_L"))
    res_R, res_L, p_R, p_L = s["res_R"], s["res_L"], s["p_R"], s["p_L"]
    out = P.guided_dock(xR, xL, res_R, res_L, p_R, p_L, n_rot=256, cone=60.0, top=10)
    # the pieces, by hand
    centres = []
    for x, res, p in ((s["xyz_R"], res_R, p_R), (s["xyz_L"], res_L, p_L)):
        x64, p64 = x.astype(np.float64), p.astype(np.float64)
        cen = np.stack([x64[res == r].mean(0) for r in range(int(res.max()) + 1)])
        centres.append(((p64[:, None] * cen).sum(0) / p64.sum(), x64.mean(0)))
    (cif_R, c_R), (cif_L, c_L) = centres
    got_R, got_L = P._centres(s["xyz_R"], res_R, int(res_R.max()) + 1, p_R, "receptor"), P._centres(s["xyz_L"], res_L, int(res_L.max()) + 1, p_L, "ligand")
    assert all(np.abs(a - b).max() <= 1e-12 for a, b in zip(got_R + got_L, (cif_R, c_R, cif_L, c_L)))
    (cif_R, c_R), (cif_L, c_L) = got_R, got_L
    u = (cif_R - c_R) / np.sqrt(((cif_R - c_R) ** 2).sum())
    rots, keep = P.cone_filter(256, cif_L - c_L, u, 60.0)
    assert out.n_sampled == keep.size and 0 < keep.size < 256
    origins = P.poses_about(rots, c_L, cif_R)
    sl, t, _ = P.slide_to_contact(xR, xL, rots, origins, np.tile(u.astype(np.float32), (keep.size, 1)))
    hits = np.nonzero(~np.isnan(host(sl)))[0]
    assert hits.size > 10
    sc = P.pose_scores(xR, xL, res_R, res_L, rots[hits], host(t)[hits], p_R, p_L)
    best = host(P.top_poses(sc.score, 10, sc.n_clash, 0))
    assert best.size == 10 and not host(sc.n_clash)[best].any()
    assert np.array_equal(host(out.index), hits[best]) and same_bits(out.rotations, rots[hits][best]) and same_bits(out.translations, host(t)[hits][best])
    assert all(x is None and y is None or same_bits(x, host(y)[best]) for x, y in zip(out.scores, sc))
    assert (out.scores.score.is_cuda and out.index.is_cuda and out.rotations.is_cuda) if on_device else isinstance(out.scores.score, np.ndarray)
    assert (np.diff(host(out.scores.score)) <= 0).all()


def test_bits_repeat_from_call_to_call_between_the_two_sides_and_for_a_pose_alone():
    from pesto_amd import poses as P
    s = sweep_system(*BIG)
    args = sweep_args(s)
    a = P.pose_scores(*args, masks=True)
    b = P.pose_scores(*args, masks=True)
    c = P.pose_scores(*(dev(v) for v in args), masks=True)
    e = P.pose_scores(dev(args[0]), *args[1:], masks=True)              # a device lead, everything else from the host
    assert same_scores(a, b) and same_scores(a, c) and same_scores(a, e) and c.score.is_cuda and e.masks.is_cuda
    sk = ("xyz_R", "xyz_L", "rotations", "translations", "directions")
    sa = P.slide_to_contact(*(s[k] for k in sk))
    sb = P.slide_to_contact(*(s[k] for k in sk))
    sc = P.slide_to_contact(*(dev(s[k]) for k in sk))
    assert all(same_bits(x, y) and same_bits(x, z) for x, y, z in zip(sa, sb, sc))
    ya = P.materialize(s["xyz_L"], s["rotations"], s["translations"])
    assert same_bits(ya, P.materialize(dev(s["xyz_L"]), dev(s["rotations"]), dev(s["translations"])))
    busiest = int(np.argmax(host(a.n_contact)))
    for f in (0, 64, busiest, 256):                                      # pose f alone gives the bits it has in the batch
        one = P.pose_scores(*args[:4], args[4][f:f + 1], args[5][f:f + 1], *args[6:], masks=True)
        assert all(same_bits(x, y[f:f + 1]) for x, y in zip(one, a)), f
        so = P.slide_to_contact(s["xyz_R"], s["xyz_L"], s["rotations"][f:f + 1], s["translations"][f:f + 1], s["directions"][f:f + 1])
        assert all(same_bits(x, y[f:f + 1]) for x, y in zip(so, sa)), f
    score = host(a.score)
    assert same_bits(P.top_poses(score, 50, host(a.n_clash), 5), P.top_poses(dev(score), 50, dev(host(a.n_clash)), 5))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_refused_call_writes_nothing(on_device):
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    from pesto_amd.trajectory import _residue_order
    c = tiny()
    F, N_R, N_L = 5, 3, 4
    model, lib = _default_model(0), _lib.load()
    place = (lambda a: dev(a)) if on_device else (lambda a: np.ascontiguousarray(a))
    side = _lib.Side(place(c["xyz_R"]), model._gpu)
    perm, off, _ = _residue_order(c["res_L"], N_L, "res_L")
    good = dict(xyz_R=c["xyz_R"], xyz_L=c["xyz_L"], res_R=c["res_R"], perm=perm, off=off, rot=c["rotations"], tr=c["translations"], p_R=c["p_R"],
                p_L=c["p_L"], dirs=np.tile(np.array([1, 0, 0], np.float32), (F, 1)))
    kinds = (np.int32,) * 5 + (np.float64,) * 3 + (np.float32, np.uint32)

    def scores(**bad):
        v = {k: place(a) for k, a in dict(good, **bad).items()}
        outs = [place(np.full((F, 2) if dt == np.uint32 else F, 7, dt)) for dt in kinds]
        rc = lib.pesto_poses_scores(model.handle, F, N_R, N_L, 2, 2, *(side.ptr(v[k]) for k in ("xyz_R", "xyz_L", "res_R", "perm", "off", "rot", "tr",
                                                                                                 "p_R", "p_L")), 5.0, 3.0, 1.0,
                                    *(side.ptr(o) for o in outs), side.kind, side.stream)
        return rc, [host(o) for o in outs]

    def slide(**bad):
        v = {k: place(a) for k, a in dict(good, **bad).items()}
        outs = [place(np.full(F, 7, np.float64)), place(np.full((F, 3), 7, np.float32)), place(np.full((F, 2), 7, np.int32))]
        rc = lib.pesto_poses_slide(model.handle, F, N_R, N_L, *(side.ptr(v[k]) for k in ("xyz_R", "xyz_L", "rot", "tr", "dirs")), 2.0, 1.0,
                                   *(side.ptr(o) for o in outs), side.kind, side.stream)
        return rc, [host(o) for o in outs]

    def frames(**bad):
        v = {k: place(a) for k, a in dict(good, **bad).items()}
        out = place(np.full((F, N_R + N_L, 3), 7, np.float32))
        rc = lib.pesto_poses_materialize(model.handle, F, N_R, N_L, *(side.ptr(v[k]) for k in ("xyz_R", "xyz_L", "rot", "tr")), side.ptr(out), side.kind,
                                         side.stream)
        return rc, [host(out)]

    over = lambda a, k, v: np.concatenate([a[:k], [v], a[k + 1:]]).astype(a.dtype)
    rc, outs = scores()
    assert rc == 0 and outs[0].tolist() == TINY["n_contact"] and outs[9].view(np.uint32).tolist() == TINY["masks"]
    bad_rot, bad_tr = c["rotations"].copy(), c["translations"].copy()
    bad_rot[4, 2, 2], bad_tr[1, 0] = np.nan, np.inf
    for bad, msg in ((dict(res_R=over(c["res_R"], 1, 2)), b"res_R"), (dict(res_R=over(c["res_R"], 0, -1)), b"res_R"), (dict(perm=over(perm, 3, N_L)), b"perm_L"),
                     (dict(off=np.array([0, 0, 4], np.int32)), b"off_L"), (dict(off=np.array([0, 2, 5], np.int32)), b"off_L"),
                     (dict(off=np.array([1, 2, 4], np.int32)), b"off_L"), (dict(p_R=np.array([0.5, -1], np.float32)), b"probabilities"),
                     (dict(p_L=np.array([np.nan, 0.5], np.float32)), b"probabilities"), (dict(rot=bad_rot), b"finite"), (dict(tr=bad_tr), b"finite")):
        rc, outs = scores(**bad)
        assert rc == -1 and msg in lib.pesto_poses_last_error(), (bad, lib.pesto_poses_last_error())
        assert all((o == 7).all() for o in outs), bad
    assert scores()[0] == 0                                                # a valid call on the same handle works straight after
    rc, outs = slide()
    assert rc == 0 and not np.isnan(outs[0]).all()
    long_dir, no_dir = good["dirs"].copy(), good["dirs"].copy()
    long_dir[2], no_dir[4] = [1.01, 0, 0], [np.nan, 0, 0]
    for bad, msg in ((dict(dirs=long_dir), b"unit length"), (dict(dirs=no_dir), b"unit length"), (dict(rot=bad_rot), b"finite"), (dict(tr=bad_tr), b"finite")):
        rc, outs = slide(**bad)
        assert rc == -1 and msg in lib.pesto_poses_last_error() and all((o == 7).all() for o in outs), bad
    assert slide()[0] == 0
    rc, outs = frames()
    assert rc == 0 and same_bits(outs[0][:, N_R:], place_def(c["xyz_L"], c["rotations"], c["translations"]))
    for bad in (dict(rot=bad_rot), dict(tr=bad_tr)):
        rc, outs = frames(**bad)
        assert rc == -1 and b"finite" in lib.pesto_poses_last_error() and (outs[0] == 7).all(), bad
    assert frames()[0] == 0
    # pesto_poses_top refuses on the host: a negative k, no poses
    score, index, n = place(np.array([0.5, 0.25, 0.75, 0.5, 0.0], np.float32)), place(np.full(F, 7, np.int32)), ctypes.c_int64(7)
    for FF, k in ((F, -1), (0, 2), (2 ** 23 + 1, 2)):
        assert lib.pesto_poses_top(model.handle, FF, k, side.ptr(score), None, 0, side.ptr(index), ctypes.byref(n), side.kind, side.stream) == -1
        assert (host(index) == 7).all() and n.value == 7
    assert lib.pesto_poses_top(model.handle, F, 3, side.ptr(score), None, 0, side.ptr(index), ctypes.byref(n), side.kind, side.stream) == 0
    assert n.value == 3 and host(index).tolist() == [2, 0, 3, 7, 7]
