"""CPU checks of the hydrogen-bond fixture (tests/golden/make_hbonds_golden.py) and of the host side of pesto_amd.hbonds: a NumPy
restatement of each definition of the module docstring reproduces the recorded lists, counts, images and shifted coordinates exactly, the
planted cases land where the definitions say, hbond_tables gives the recorded tables, bad arguments raise ValueError before any launch, and
the header's new symbols are declared with their citation, exported and bound. The restatements are the yardsticks of the GPU tests
(tests/test_hbonds.py); the generator records what they give after asserting that the reference's own hydrogen_bonds and unwrap_pbc,
run on stubs written from the text of the definitions, agree with them."""
import gzip
import math
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, golden

DONOR_TILE = 32                         # PESTO_HBONDS_DONOR_TILE, the T of the `tiles` system
SCAN_BLOCK = 1024                       # LIST_SCAN_NT of pesto_scan.h, and more than the 256-thread frame scan
TILE_P = (1, DONOR_TILE - 1, DONOR_TILE, DONOR_TILE + 1)
TILE_A = (1, 63, 64, 65, 129)
FREQS = (0.0, 0.1, 0.5, 0.9)
SYSTEMS = ["frames", "size", "planted"] + [f"tiles_{p}_{a}" for p in TILE_P for a in TILE_A]
UNWRAP = ["unwrap", "uplanted"]


# ------------------------------------------------------------------ the fixture's systems
def system(g, name):
    """dict of one system: xyz float32 [F, N, 3] (nanometres, scale 10), dh, acc, group (int8 [N]; R = 1, L = 2), the criteria"""
    if name.startswith("tiles_"):
        P, A = (int(v) for v in name.split("_")[1:])
        p0, a0 = (int(v) for v in g["tiles_start"])
        s = system(g, "frames")
        s["dh"], s["acc"] = s["dh"][p0:p0 + P], s["acc"][a0:a0 + A]
        assert s["dh"].shape[0] == P and s["acc"].shape[0] == A
        return s
    r_thr, angle = (float(v) for v in g[name + "_criteria"])
    src = "frames" if name == "size" else name
    return dict(xyz=g[name + "_xyz"], dh=g[src + "_dh"].astype(np.int32), acc=g[src + "_acc"].astype(np.int32), group=g[src + "_group"].astype(np.int8),
                r_thr=r_thr, angle=angle)


def unwrap_system(g, name):
    return dict(xyz=g[name + "_xyz"], box=g[name + "_box"], mol=g[name + "_mol"].astype(np.int32), masses=g[name + "_masses"].astype(np.float64))


# ------------------------------------------------------------------ the definitions (NumPy; every operation rounded on its own)
def bonded_def(x, dh, acc, r_thr=2.5, angle=120.0, scale=10.0):
    """(bonded bool [P, A], d float32 [P, A]) of ONE frame x float32 [N, 3]"""
    D, H, Ac = x[dh[:, 0]], x[dh[:, 1]], x[acc]
    with np.errstate(invalid="ignore"):
        dx, dy, dz = (H[:, None, c] - Ac[None, :, c] for c in range(3))
        d = np.sqrt((dx * dx + dy * dy) + dz * dz) * np.float32(scale)
        near = d < np.float32(r_thr)
        u = (D.astype(np.float64) - H.astype(np.float64))[:, None, :]
        v = Ac.astype(np.float64)[None, :, :] - H.astype(np.float64)[:, None, :]
        c = (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]
        uu = (u[..., 0] * u[..., 0] + u[..., 1] * u[..., 1]) + u[..., 2] * u[..., 2]
        vv = (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]
        k = math.cos(math.radians(angle)) ** 2
        ok = (c < 0) & (c * c > k * (uu * vv))
    return near & ok & (acc[None, :] != dh[:, :1]), d


def frame_hbonds_def(xyz, dh, acc, r_thr=2.5, angle=120.0, scale=10.0, group=None):
    """(offsets int64 [F + 1], triplets int32 [K, 3], d float32 [K]) in candidate order per frame"""
    off, trip, dd = [0], [], []
    for x in xyz:
        b, d = bonded_def(x, dh, acc, r_thr, angle, scale)
        if group is not None:
            gd, ga = group[dh[:, 0]][:, None], group[acc][None, :]
            b &= (gd != 0) & (ga != 0) & (gd != ga)
        p, a = np.nonzero(b)
        trip.append(np.stack([dh[p, 0], dh[p, 1], acc[a]], 1))
        dd.append(d[p, a])
        off.append(off[-1] + p.size)
    return np.array(off, np.int64), np.concatenate(trip).astype(np.int32).reshape(-1, 3), np.concatenate(dd).astype(np.float32)


def occupancy_def(xyz, dh, acc, freq, r_thr=2.5, angle=120.0, scale=10.0):
    """(triplets int32 [k, 3], counts int32 [k]): float(n) / float(F) > freq, in candidate order"""
    n = np.zeros((dh.shape[0], acc.shape[0]), np.int64)
    for x in xyz:
        n += bonded_def(x, dh, acc, r_thr, angle, scale)[0]
    keep = (n.astype(np.float64) / float(xyz.shape[0]) > freq) & (acc[None, :] != dh[:, :1])
    p, a = np.nonzero(keep)
    return np.stack([dh[p, 0], dh[p, 1], acc[a]], 1).astype(np.int32).reshape(-1, 3), n[p, a].astype(np.int32)


def hydrogen_bonds_def(xyz, dh, acc, group, r_thr=2.5, angle=120.0, scale=10.0):
    """(nhb float64 [F], rows): per frame the group-filtered triplets, donor in L (2) first, then donor in R (1)"""
    off, trip, _ = frame_hbonds_def(xyz, dh, acc, r_thr, angle, scale, group)
    rows = []
    for f in range(off.size - 1):
        t = trip[off[f]:off[f + 1]]
        rows.append(np.concatenate([t[group[t[:, 0]] == 2], t[group[t[:, 0]] == 1]]))
    return np.diff(off).astype(np.float64), rows


IMAGES = np.array([(gx, gy, gz) for gy in (0.0, 1.0, -1.0) for gx in (0.0, 1.0, -1.0) for gz in (0.0, 1.0, -1.0)])      # y slowest, x, z fastest


def com_def(xyz, mol, masses):
    """float64 [F, M, 3]: the mass-weighted mean of every molecule"""
    M = int(mol.max()) + 1
    x = xyz.astype(np.float64)
    return np.stack([(masses[mol == m, None] * x[:, mol == m]).sum(1) / masses[mol == m].sum() for m in range(M)], 1)


def unwrap_def(xyz, box, mol, masses):
    """(shifted float32 [F, N, 3], image int32 [F, M], gap float64 [F, M]: the relative distance gap between the two nearest images)"""
    com = com_def(xyz, mol, masses)
    F, M = com.shape[:2]
    L = box.astype(np.float64)
    out, image, gap = xyz.copy(), np.zeros((F, M), np.int32), np.full((F, M), np.inf)
    for f in range(F):
        for m in range(1, M):
            if np.isnan(com[f, m]).any() or np.isnan(com[f, 0]).any() or np.isnan(L[f]).any():
                continue
            t = (com[f, m][None] + L[f][None] * IMAGES) - com[f, 0][None]
            dist = np.sqrt((t[:, 0] * t[:, 0] + t[:, 1] * t[:, 1]) + t[:, 2] * t[:, 2])
            k = int(np.argmin(dist))                    # (the first minimum)
            two = np.sort(dist)[:2]
            gap[f, m] = (two[1] - two[0]) / max(two[0], 1e-300)
            image[f, m] = k
            sel = mol == m
            out[f, sel] = (xyz[f, sel].astype(np.float64) + (L[f] * IMAGES[k])[None]).astype(np.float32)
    return out, image, gap


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def read_structure(name):
    from pesto_amd import structure_io
    return structure_io.Structure.parse_pdb(gzip.open(os.path.join(GOLDEN, "pdb", name + ".gz"), "rt").read()).to_dict()


# ------------------------------------------------------------------ the recorded outputs against the restatements
@pytest.mark.parametrize("name", SYSTEMS)
def test_restatement_reproduces_the_recorded_lists(name):
    g = golden("hbonds")
    s = system(g, name)
    off, trip, d = frame_hbonds_def(s["xyz"], s["dh"], s["acc"], s["r_thr"], s["angle"])
    assert np.array_equal(off, g[name + "_off"]) and np.array_equal(trip, g[name + "_trip"].astype(np.int32).reshape(-1, 3))
    assert same_bits(d, g[name + "_d"])
    goff, gtrip, _ = frame_hbonds_def(s["xyz"], s["dh"], s["acc"], s["r_thr"], s["angle"], group=s["group"])
    assert np.array_equal(goff, g[name + "_goff"]) and np.array_equal(gtrip, g[name + "_gtrip"].astype(np.int32).reshape(-1, 3))
    if name.startswith("tiles_"):
        return
    for freq in FREQS:
        t, n = occupancy_def(s["xyz"], s["dh"], s["acc"], freq, s["r_thr"], s["angle"])
        assert np.array_equal(t, g[f"{name}_occ{freq}_trip"].astype(np.int32).reshape(-1, 3)) and np.array_equal(n, g[f"{name}_occ{freq}_n"]), freq
    nhb, rows = hydrogen_bonds_def(s["xyz"], s["dh"], s["acc"], s["group"], s["r_thr"], s["angle"])
    assert np.array_equal(nhb, g[name + "_nhb"]) and np.array_equal(np.concatenate(rows), g[name + "_ihb"].astype(np.int32).reshape(-1, 3))


def test_frames_system_pins_the_strict_occupancy_comparison_and_the_scan_block():
    g = golden("hbonds")
    s = system(g, "frames")
    F = s["xyz"].shape[0]
    t0, n0 = occupancy_def(s["xyz"], s["dh"], s["acc"], 0.0)
    assert F == 16 and np.any(2 * n0 == F)                                      # occupancy exactly 0.5: out at freq = 0.5
    assert g["frames_occ0.5_n"].min() > F // 2 and n0.min() >= 1
    assert g["frames_occ0.0_n"].size > g["frames_occ0.1_n"].size > g["frames_occ0.5_n"].size > g["frames_occ0.9_n"].size > 0
    assert 0 < g["frames_goff"][-1] < g["frames_off"][-1]
    n = np.diff(g["size_off"])
    assert n.max() > SCAN_BLOCK and n[int(g["size_empty_frame"])] == 0 and 0 < int(g["size_empty_frame"]) < n.size - 1
    # the tile crops straddle the donor tile and the 64-lane acceptor walk, each with a bond
    assert all(g[f"tiles_{p}_{a}_off"][-1] > 0 for p in TILE_P for a in TILE_A)


def test_planted_cases_land_where_the_definitions_say():
    g = golden("hbonds")
    s = system(g, "planted")
    assert s["xyz"].shape[1] <= 64
    role = {str(k): int(v) for k, v in zip(g["planted_roles"], g["planted_role_atoms"])}
    frame = int(g["planted_frame"])
    off, trip, d = frame_hbonds_def(s["xyz"], s["dh"], s["acc"])
    per_frame = np.diff(off)
    assert per_frame[0] == 0 and per_frame[-1] == 0 and np.any(per_frame[1:-1] == 0) and per_frame.max() > 0
    listed = {tuple(t) for t in trip[off[frame]:off[frame + 1]].tolist()}
    acceptors_of = lambda don: sorted(a for dd, _, a in listed if dd == role[don])      # noqa: E731
    # the distance: at r_thr / scale out, one float32 below in, one above out
    b, dist = bonded_def(s["xyz"][frame], s["dh"], s["acc"])
    col = {int(a): k for k, a in enumerate(s["acc"])}
    row = {int(dn): k for k, dn in enumerate(s["dh"][:, 0])}
    at, below, above = (dist[row[role["D_dist"]], col[role[k]]] for k in ("A_at", "A_below", "A_above"))
    assert at == np.float32(2.5) and below == np.nextafter(np.float32(2.5), np.float32(0)) and above == np.nextafter(np.float32(2.5), np.float32(9))
    assert acceptors_of("D_dist") == [role["A_below"]]
    # the angle: 119.9 degrees out, 120.1 in
    assert acceptors_of("D_angle") == [role["A_1201"]]
    for key, want in (("A_1199", 119.9), ("A_1201", 120.1)):
        x = s["xyz"][frame].astype(np.float64)
        u, v = x[role["D_angle"]] - x[role["H_angle"]], x[role[key]] - x[role["H_angle"]]
        assert abs(math.degrees(math.acos(u @ v / math.sqrt((u @ u) * (v @ v)))) - want) < 0.02
    # the donor itself is an acceptor and never listed; an acceptor on H (vv = 0), a donor on its H (uu = 0), a NaN acceptor: out
    assert role["D_self"] in s["acc"] and all(a != dd for dd, _, a in listed)
    assert acceptors_of("D_self") == [] and acceptors_of("D_uu0") == [] and acceptors_of("D_nan") == []
    assert np.array_equal(s["xyz"][frame][role["A_onH"]], s["xyz"][frame][role["H_self"]])
    assert np.array_equal(s["xyz"][frame][role["D_uu0"]], s["xyz"][frame][role["H_uu0"]]) and np.isnan(s["xyz"][frame][role["A_nan"]]).any()
    # one donor bonded to two acceptors
    assert acceptors_of("D_two") == sorted([role["A_two0"], role["A_two1"]])
    # the group filter: an acceptor of group 0 and one of the donor's own group drop out
    assert (s["group"] == 0).any()
    goff, gtrip, _ = frame_hbonds_def(s["xyz"], s["dh"], s["acc"], group=s["group"])
    assert 0 < goff[-1] < off[-1]


def test_no_recorded_decision_is_within_rounding_of_its_threshold():
    """every decision within 1e-6 (relative) of its threshold is a planted one"""
    g = golden("hbonds")
    for name in ("frames", "size", "planted"):
        s = system(g, name)
        n_d = n_a = 0
        k = math.cos(math.radians(s["angle"])) ** 2
        for x in s["xyz"]:
            _, d = bonded_def(x, s["dh"], s["acc"], s["r_thr"], s["angle"])
            with np.errstate(invalid="ignore"):
                n_d += int((np.abs(d.astype(np.float64) - s["r_thr"]) <= 1e-6 * s["r_thr"]).sum())
                p, a = np.nonzero(d < np.float32(1.01 * s["r_thr"]))
                u = x[s["dh"][p, 0]].astype(np.float64) - x[s["dh"][p, 1]].astype(np.float64)
                v = x[s["acc"][a]].astype(np.float64) - x[s["dh"][p, 1]].astype(np.float64)
                c, uu, vv = (u * v).sum(1), (u * u).sum(1), (v * v).sum(1)
                n_a += int(((c < 0) & (np.abs(c * c - k * uu * vv) <= 1e-6 * k * uu * vv) & (uu > 0) & (vv > 0)).sum())
        planted = name == "planted"
        assert n_a == 0 and (n_d > 0 if planted else n_d == 0), (name, n_d, n_a)
        F = s["xyz"].shape[0]
        _, n0 = occupancy_def(s["xyz"], s["dh"], s["acc"], 0.0, s["r_thr"], s["angle"])
        for freq in FREQS:
            close, exact = np.abs(n0 / F - freq) <= 1e-6, n0 / F == freq       # (an exact tie is a planted decision: 2 n = F at freq 0.5)
            assert not np.any(close & ~exact) and (not exact.any() or (freq == 0.5 and F % 2 == 0)), (name, freq)
    for name in UNWRAP:
        s = unwrap_system(g, name)
        gap = unwrap_def(s["xyz"], s["box"], s["mol"], s["masses"])[2]
        ties = np.argwhere(gap <= 1e-6)
        assert ties.tolist() == (g["uplanted_ties"].tolist() if name == "uplanted" else []), (name, ties)


@pytest.mark.parametrize("name", UNWRAP)
def test_unwrap_restatement_reproduces_the_recorded_images_and_coordinates(name):
    g = golden("hbonds")
    s = unwrap_system(g, name)
    out, image, _ = unwrap_def(s["xyz"], s["box"], s["mol"], s["masses"])
    assert np.array_equal(image, g[name + "_image"]) and same_bits(out, g[name + "_out"])
    moved = np.array([(g[name + "_image"][:, m] != 0).any() for m in range(image.shape[1])])
    assert not moved[0] and moved[1:].any()
    if name == "unwrap":
        assert np.bincount(s["mol"]).min() == 1 and image.shape == (4, 4) and np.unique(image[:, 1:]).size > 4
        assert np.array_equal(s["masses"], __import__("pesto_amd.hbonds").hbonds.atomic_masses(read_structure("1ZNS_ion.pdb")["element"]))
    else:
        # an equidistant pair of images resolves to the first in (y, x, z) order; a NaN box length and a NaN atom leave their frames alone
        f, m = g["uplanted_ties"][0]
        assert image[f, m] == 6 and np.array_equal(IMAGES[6], (-1.0, 0.0, 0.0))
        nan_box = int(np.nonzero(np.isnan(s["box"]).any(1))[0][0])
        assert not image[nan_box].any() and same_bits(out[nan_box], s["xyz"][nan_box])
        assert np.any(np.diff(np.nonzero(s["mol"] == 1)[0]) > 1)               # rows that are not contiguous
        fn, an = np.argwhere(np.isnan(s["xyz"]).any(2))[0]
        assert image[fn, s["mol"][an]] == 0 and image[fn].any()


# ------------------------------------------------------------------ the host side of pesto_amd.hbonds
def test_hbond_tables_on_6I9F_and_water():
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    st = read_structure("6I9F.pdb")
    dh, acc = H.hbond_tables(st)
    assert dh.dtype == np.int32 and acc.dtype == np.int32 and dh.shape == (320, 2) and acc.shape == (476,)
    keep = g["frames_atoms"].astype(np.int64)                   # the fixture keeps the atoms of the tables only, renumbered
    assert np.array_equal(keep[g["frames_dh"].astype(np.int64)], dh) and np.array_equal(keep[g["frames_acc"].astype(np.int64)], acc)
    assert np.array_equal(dh, np.array(sorted(map(tuple, dh.tolist())))) and np.all(np.diff(acc) > 0)
    el = np.char.upper(np.asarray(st["element"]))
    assert np.all(np.isin(el[dh[:, 0]], ("N", "O"))) and np.all(el[dh[:, 1]] == "H") and np.all(np.isin(el[acc], ("N", "O")))
    bond = np.linalg.norm(st["xyz"][dh[:, 0]].astype(np.float64) - st["xyz"][dh[:, 1]], axis=1)
    assert bond.max() <= 1.09 + 1e-3
    assert H.hbond_tables(st, max_bond=0.5)[0].shape == (0, 2)
    # two waters beside a hydroxyl: left out of both tables when asked
    w = dict(xyz=np.array([[0, 0, 0], [0.96, 0, 0], [5, 0, 0], [5.96, 0, 0], [4.76, 0.93, 0], [9, 0, 0], [9.9, 0, 0]], np.float32),
             element=np.array(["O", "H", "O", "H", "H", "O", "D"]), resname=np.array(["SER", "SER", "HOH", "HOH", "HOH", "DOD", "DOD"]),
             resid=np.array([1, 1, 2, 2, 2, 3, 3]), chain_name=np.array(["A"] * 7), name=np.array(["OG", "HG", "O", "H1", "H2", "O", "D1"]))
    dh, acc = H.hbond_tables(w)
    assert dh.tolist() == [[0, 1]] and acc.tolist() == [0]
    dh, acc = H.hbond_tables(w, exclude_water=False)
    assert dh.tolist() == [[0, 1], [2, 3], [2, 4], [5, 6]] and acc.tolist() == [0, 2, 5]


def test_atomic_masses():
    from pesto_amd import hbonds as H
    need = ["H", "D", "C", "N", "O", "F", "Na", "Mg", "P", "S", "Cl", "K", "Ca", "Mn", "Fe", "Co", "Ni", "Cu", "Zn", "Se", "Br", "I"]
    m = H.atomic_masses(need)
    assert m.dtype == np.float64 and np.all(m > 0) and abs(m[2] - 12.011) < 1e-3 and abs(m[18] - 65.38) < 1e-2 and m[1] > m[0]
    assert np.array_equal(H.atomic_masses(["ZN", " zn", "Zn "]), np.full(3, m[18]))
    with pytest.raises(ValueError):
        H.atomic_masses(["C", "Xx"])


def test_bad_arguments_raise_before_any_launch():
    from pesto_amd import hbonds as H
    no = object()                                               # a model without a handle: reaching the launch raises AttributeError
    x = np.zeros((2, 5, 3), np.float32)
    dh, acc = np.array([[0, 1], [2, 3]], np.int32), np.array([4, 0], np.int32)
    box, mol = np.ones((2, 3), np.float32), np.array([0, 0, 1, 1, 1])
    nan, inf = float("nan"), float("inf")
    bad_frames = [
        dict(xyz=np.zeros((2, 5, 2), np.float32)), dict(xyz=np.zeros((5,), np.float32)),
        dict(angle=89.9), dict(angle=180.0), dict(angle=nan), dict(angle=-120.0),
        dict(r_thr=nan), dict(r_thr=inf), dict(r_thr=0.0), dict(r_thr=-1.0), dict(scale=nan), dict(scale=inf), dict(scale=0.0), dict(scale=-10.0),
        dict(dh=np.array([0, 1, 2, 3], np.int32)), dict(dh=np.zeros((2, 3), np.int32)), dict(dh=np.zeros((0, 2), np.int32)),
        dict(dh=np.array([[0, -1], [2, 3]])), dict(dh=np.array([[0, 5], [2, 3]])), dict(dh=np.array([[0.0, 1.0], [2.0, 3.0]])),
        dict(acc=np.array([4, 5])), dict(acc=np.array([-1])), dict(acc=np.array([1.5])), dict(acc=np.zeros((1, 1), np.int32)), dict(acc=np.zeros(0, np.int32)),
        dict(group=np.zeros(4, np.int8)), dict(group=np.full(5, -1)), dict(group=np.zeros(5)), dict(capacity=0), dict(capacity=2 ** 30),
        dict(xyz=np.broadcast_to(np.float32(0), (H.MAX_FRAMES + 1, 5, 3))),
        dict(xyz=np.broadcast_to(np.float32(0), (2 ** 19, 5, 3)), dh=np.broadcast_to(np.int32(0), (32 * 32 + 1, 2))),    # F * ceil(P / 32) = 2^24 + 2^19
        dict(dh=np.broadcast_to(np.int32(0), (2 ** 16, 2)), acc=np.broadcast_to(np.int32(1), (2 ** 15,))),            # P * A = 2^31
    ]
    for kw in bad_frames:
        args = dict(xyz=x, dh=dh, acc=acc, model=no)
        args.update(kw)
        with pytest.raises(ValueError):
            H.frame_hbonds(**args)
        if not {"group", "capacity"} & set(kw) and args["xyz"].shape[0] != 2 ** 19:      # (what baker_hubbard takes and limits too)
            with pytest.raises(ValueError):
                H.baker_hubbard(**args)
    for freq in (nan, inf, -0.1):
        with pytest.raises(ValueError):
            H.baker_hubbard(x, dh, acc, freq=freq, model=no)
    for kw in (dict(ids_R=[0, 1], ids_L=[1, 2]), dict(ids_R=[0, 9], ids_L=[1]), dict(ids_R=[], ids_L=[1]), dict(ids_R=[0], ids_L=[1], angle=10.0)):
        with pytest.raises(ValueError):
            H.hydrogen_bonds(x, dh, acc, model=no, **kw)
    ok = np.ones(5)
    bad_unwrap = [
        dict(xyz=np.zeros((5, 3), np.float32)), dict(unitcell_lengths=np.ones((3, 3), np.float32)), dict(unitcell_lengths=np.ones((2, 2), np.float32)),
        dict(mol=np.array([0, 0, 2, 2, 2])), dict(mol=np.array([0, 0, 1, 1])), dict(mol=np.array([0, -1, 1, 1, 1])), dict(mol=np.array([0.0, 0, 1, 1, 1])),
        dict(masses=np.array([1, 1, 0, 1, 1.0])), dict(masses=np.array([1, 1, -2, 1, 1.0])), dict(masses=np.array([1, 1, nan, 1, 1.0])),
        dict(masses=np.array([1, 1, inf, 1, 1.0])), dict(masses=np.ones(4)), dict(masses=None), dict(elements=["C"] * 5),
        dict(masses=None, elements=["C", "C", "Qq", "C", "C"]), dict(xyz=np.broadcast_to(np.float32(0), (H.MAX_FRAMES + 1, 5, 3))),
    ]
    for kw in bad_unwrap:
        args = dict(xyz=x, unitcell_lengths=box, mol=mol, masses=ok, model=no)
        args.update(kw)
        if args["xyz"].shape[0] > 2 and "unitcell_lengths" not in kw:
            args["unitcell_lengths"] = np.broadcast_to(np.float32(1), (args["xyz"].shape[0], 3))
        with pytest.raises(ValueError):
            H.unwrap_pbc(**args)
    # valid arguments get as far as the handle
    for call in (lambda: H.frame_hbonds(x, dh, acc, model=no), lambda: H.baker_hubbard(x, dh, acc, model=no),
                 lambda: H.hydrogen_bonds(x, dh, acc, [0, 1], [2, 3, 4], model=no), lambda: H.unwrap_pbc(x, box, mol, ok, model=no),
                 lambda: H.unwrap_pbc(x, box, mol, elements=["C", "N", "O", "H", "Zn"], model=no)):
        with pytest.raises(AttributeError):
            call()


def test_symbols_are_declared_with_their_citation_exported_and_bound():
    import pesto_amd
    from pesto_amd import _lib
    from pesto_amd import hbonds as H
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    lib = _lib.load()
    for name in ("pesto_frame_hbonds", "pesto_hbond_occupancy", "pesto_unwrap_pbc"):
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int " + name + r"\(", hdr, re.S)
        assert m and "replaces:" in m.group(1) and re.search(r"trajectory_utils\.py:\d+-\d+", m.group(1)), name
        assert name in _lib.ABI_SYMBOLS and getattr(lib, name).argtypes and getattr(lib, name).restype is not None
    assert "pesto_hbonds_last_error" in _lib.ABI_SYMBOLS and re.search(r"const char\* pesto_hbonds_last_error\(void\);", hdr)
    assert lib.pesto_hbonds_last_error.restype is not None and lib.pesto_hbonds_last_error() is not None
    enum = {k: v for k, v in re.findall(r"PESTO_HBONDS_(\w+) = ([^,/\n]+)", hdr)}
    val = {k: int(eval(v.strip(), {"__builtins__": {}})) for k, v in enum.items()}      # (integer constant expressions of the header)
    assert val == dict(MAX_FRAMES=H.MAX_FRAMES, MAX_PAIRS=H.MAX_PAIRS, MAX_LIST=H.MAX_LIST, DONOR_TILE=H.DONOR_TILE)
    assert H.DONOR_TILE == DONOR_TILE and int(golden("hbonds")["donor_tile"]) == DONOR_TILE
    for name in ("hbonds", "frame_hbonds", "baker_hubbard", "hydrogen_bonds", "unwrap_pbc", "atomic_masses", "hbond_tables"):
        assert name in pesto_amd.__all__ and getattr(pesto_amd, name) is (H if name == "hbonds" else getattr(H, name))
    # the entry points check their arguments before they touch a device
    x = np.zeros((1, 3, 3), np.float32)
    sz = np.zeros(1, np.int64)
    assert lib.pesto_frame_hbonds(None, 1, 3, 1, 1, x.ctypes.data, None, None, None, 2.5, 10.0, 0.25, 16, None, None, None, sz.ctypes.data, 0, None) == -1
    assert lib.pesto_hbonds_last_error() == b"bad arguments"
