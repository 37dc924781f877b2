"""GPU tests of pesto_amd.hbonds (pesto_hbonds.hip) against the definitions of its module docstring, whose NumPy restatements
(tests/test_hbonds_fixture.py) reproduce tests/golden/hbonds.npz: frame lists, occupancy lists and images exactly, d and the shifted
coordinates bit for bit, through host arrays and ROCm tensors, with the group filter, the capacity protocol and identical bits from call
to call; unwrap_pbc followed by frame_hbonds on the same ROCm tensor."""
import math

import numpy as np
import pytest

from conftest import golden
from test_hbonds_fixture import FREQS, SCAN_BLOCK, SYSTEMS, UNWRAP, frame_hbonds_def, occupancy_def, system, unwrap_def, unwrap_system

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def on_side(on_device, *got):
    return all(v.is_cuda for v in got) if on_device else all(isinstance(v, np.ndarray) for v in got)


def check_lists(g, name, got, keys=("off", "trip", "d"), on_device=False):
    off, trip, d = got
    assert on_side(on_device, *got)
    assert host(off).dtype == np.int64 and host(trip).dtype == np.int32 and host(d).dtype == np.float32
    assert np.array_equal(host(off), g[f"{name}_{keys[0]}"]), name
    want = g[f"{name}_{keys[1]}"].astype(np.int32).reshape(-1, 3)
    assert host(trip).shape == want.shape and np.array_equal(host(trip), want), name
    if keys[2]:
        assert np.array_equal(host(d).view(np.uint32), g[f"{name}_{keys[2]}"].view(np.uint32)), name


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_frame_hbonds(name, on_device):
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    s = system(g, name)
    xyz = dev(s["xyz"]) if on_device else s["xyz"]
    crit = dict(r_thr=s["r_thr"], angle=s["angle"])
    got = H.frame_hbonds(xyz, s["dh"], s["acc"], **crit)
    check_lists(g, name, got, on_device=on_device)
    again = H.frame_hbonds(xyz, s["dh"], s["acc"], **crit)
    assert all(same_bits(u, v) for u, v in zip(got, again))
    # the group filter: donor and acceptor in different non-zero groups
    grouped = H.frame_hbonds(xyz, s["dh"], s["acc"], group=dev(s["group"]) if on_device else s["group"], **crit)
    check_lists(g, name, grouped, ("goff", "gtrip", None), on_device)
    if name == "planted":                               # a single frame passed as [N, 3]
        f = int(g["planted_frame"])
        o, t, d = H.frame_hbonds(xyz[f], s["dh"], s["acc"])
        lo, hi = g["planted_off"][f], g["planted_off"][f + 1]
        assert host(o).tolist() == [0, hi - lo] and np.array_equal(host(t), g["planted_trip"][lo:hi].astype(np.int32))
        assert np.array_equal(host(d).view(np.uint32), g["planted_d"][lo:hi].view(np.uint32))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", ["frames", "size", "planted"])
def test_baker_hubbard_and_hydrogen_bonds(name, on_device):
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    s = system(g, name)
    xyz = dev(s["xyz"]) if on_device else s["xyz"]
    crit = dict(r_thr=s["r_thr"], angle=s["angle"])
    for freq in FREQS:
        trip, n = H.baker_hubbard(xyz, s["dh"], s["acc"], freq, return_counts=True, **crit)
        assert on_side(on_device, trip, n) and host(trip).dtype == np.int32 and host(n).dtype == np.int32
        want = g[f"{name}_occ{freq}_trip"].astype(np.int32).reshape(-1, 3)
        assert host(trip).shape == want.shape and np.array_equal(host(trip), want) and np.array_equal(host(n), g[f"{name}_occ{freq}_n"]), (name, freq)
        only = H.baker_hubbard(xyz, s["dh"], s["acc"], freq, **crit)
        assert same_bits(only, trip)
    # the reference's form: per frame the rows with the donor in L first, then the donor in R
    ids_R, ids_L = np.nonzero(s["group"] == 1)[0], np.nonzero(s["group"] == 2)[0]
    nhb, rows = H.hydrogen_bonds(xyz, s["dh"], s["acc"], ids_R, ids_L, **crit)
    assert isinstance(nhb, np.ndarray) and nhb.dtype == np.float64 and np.array_equal(nhb, g[name + "_nhb"]) and len(rows) == nhb.size
    assert on_side(on_device, *rows) and all(host(r).dtype == np.int32 and host(r).shape == (int(k), 3) for r, k in zip(rows, nhb))
    assert np.array_equal(np.concatenate([host(r) for r in rows]), g[name + "_ihb"].astype(np.int32).reshape(-1, 3))
    masks = H.hydrogen_bonds(xyz, s["dh"], s["acc"], s["group"] == 1, s["group"] == 2, **crit)
    assert np.array_equal(masks[0], nhb) and all(same_bits(u, v) for u, v in zip(masks[1], rows))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_capacity_too_small_returns_the_count_and_the_repeat_completes(on_device):
    from pesto_amd import _lib
    from pesto_amd import hbonds as H
    from pesto_amd.patches import _default_model
    g = golden("hbonds")
    s = system(g, "size")
    F, N, P, A = s["xyz"].shape[0], s["xyz"].shape[1], s["dh"].shape[0], s["acc"].shape[0]
    K = int(g["size_off"][-1])
    model = _default_model(0)
    xyz = dev(s["xyz"]) if on_device else s["xyz"]
    side = _lib.Side(xyz, model._gpu)
    dh, acc = side.put(s["dh"], np.int32), side.put(s["acc"], np.int32)
    lib = _lib.load()
    k2 = math.cos(math.radians(s["angle"])) ** 2
    for cap in (16, K - 1, K):
        off, trip, d, sz = side.empty((F + 1,), np.int64), side.empty((cap + 8, 3), np.int32), side.empty((cap + 8,), np.float32), np.zeros(1, np.int64)
        trip[cap:], d[cap:] = -7, -7.0                  # a guard behind the capacity: nothing is written beyond cap
        _lib.check(lib.pesto_frame_hbonds(model.handle, F, N, P, A, side.ptr(xyz), side.ptr(dh), side.ptr(acc), None, s["r_thr"], 10.0, float(k2), cap,
                                          side.ptr(off), side.ptr(trip), side.ptr(d), sz.ctypes.data, side.kind, side.stream), lib.pesto_hbonds_last_error)
        assert int(sz[0]) == K and np.array_equal(host(off), g["size_off"]), cap            # the count and the offsets come back either way
        assert np.all(host(trip)[cap:] == -7) and np.all(host(d)[cap:] == -7.0), cap
        if cap == K:
            check_lists(g, "size", (off, trip[:cap], d[:cap]), on_device=on_device)
    crit = dict(r_thr=s["r_thr"], angle=s["angle"])
    check_lists(g, "size", H.frame_hbonds(xyz, s["dh"], s["acc"], capacity=16, **crit), on_device=on_device)
    check_lists(g, "size", H.frame_hbonds(xyz, s["dh"], s["acc"], capacity=K, **crit), on_device=on_device)
    # the occupancy list, same protocol
    want = g["size_occ0.0_trip"].astype(np.int32).reshape(-1, 3)
    k = want.shape[0]
    for cap in (16, k - 1, k):
        trip, n, sz = side.empty((cap + 8, 3), np.int32), side.empty((cap + 8,), np.int32), np.zeros(1, np.int64)
        trip[cap:], n[cap:] = -7, -7
        _lib.check(lib.pesto_hbond_occupancy(model.handle, F, N, P, A, side.ptr(xyz), side.ptr(dh), side.ptr(acc), s["r_thr"], 10.0, float(k2), 0.0, cap,
                                             side.ptr(trip), side.ptr(n), sz.ctypes.data, side.kind, side.stream), lib.pesto_hbonds_last_error)
        assert int(sz[0]) == k and np.all(host(trip)[cap:] == -7) and np.all(host(n)[cap:] == -7), cap
        if cap == k:
            assert np.array_equal(host(trip)[:cap], want) and np.array_equal(host(n)[:cap], g["size_occ0.0_n"])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", UNWRAP)
def test_unwrap_pbc(name, on_device):
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    s = unwrap_system(g, name)
    xyz, box = (dev(s["xyz"]), dev(s["box"])) if on_device else (s["xyz"], s["box"])
    before = host(xyz).copy()
    out, image = H.unwrap_pbc(xyz, box, s["mol"], s["masses"], return_images=True)
    assert on_side(on_device, out, image) and host(image).dtype == np.int32
    assert np.array_equal(host(image), g[name + "_image"]) and same_bits(out, g[name + "_out"])
    assert same_bits(host(xyz), before)                                         # the input is never modified
    again = H.unwrap_pbc(xyz, box, s["mol"], s["masses"])
    assert same_bits(again, out)
    if name == "unwrap":                                # the masses from the element symbols
        from test_hbonds_fixture import read_structure
        assert same_bits(H.unwrap_pbc(xyz, box, s["mol"], elements=read_structure("1ZNS_ion.pdb")["element"]), out)
        assert same_bits(H.unwrap_pbc(xyz[:1], box[:1], dev(s["mol"]) if on_device else s["mol"], s["masses"]), g[name + "_out"][:1])


def test_unwrap_then_frame_hbonds_on_the_device():
    """the periodic copies of the second half of the molecule are brought back and the bonds across the halves found, ROCm tensors all the way"""
    import torch
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    s = system(g, "frames")
    xyz = s["xyz"][:4]
    mol = (s["group"] == 2).astype(np.int32)
    box = np.tile(np.array([[8.0, 9.0, 10.0]], np.float32), (4, 1))               # nanometres, wider than the molecule
    wrapped = xyz.copy()
    wrapped[:, mol == 1] += box[:, None, :] * np.array([1.0, -1.0, 0.0], np.float32)
    masses = np.ones(mol.size)
    want_x, want_k, gap = unwrap_def(wrapped, box, mol, masses)
    assert np.all(want_k[:, 1] == 15) and gap[:, 1].min() > 1e-3                  # (gx, gy, gz) = (-1, 1, 0): k = 1 * 9 + 2 * 3 + 0
    xd = dev(wrapped)
    out, image = H.unwrap_pbc(xd, dev(box), dev(mol), dev(masses), return_images=True)
    off, trip, d = H.frame_hbonds(out, dev(s["dh"]), dev(s["acc"]))
    assert out.is_cuda and image.is_cuda and off.is_cuda and trip.is_cuda and d.is_cuda and out.device == xd.device
    assert np.array_equal(host(image), want_k) and same_bits(out, want_x)
    w_off, w_trip, w_d = frame_hbonds_def(want_x, s["dh"], s["acc"])
    assert np.array_equal(host(off), w_off) and np.array_equal(host(trip), w_trip) and np.array_equal(host(d).view(np.uint32), w_d.view(np.uint32))
    assert w_off[-1] > 0 and frame_hbonds_def(wrapped, s["dh"], s["acc"])[0][-1] < w_off[-1]
    assert torch.cuda.current_device() == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_more_donor_pairs_than_the_offsets_scan_has_threads(on_device):
    """the donor table four times over (1,280 rows, every bond four times): every thread of the one workgroup that scans the donor
    pairs' totals of the occupancy list owns two of them, and the frame lists hold more than one donor tile per wave"""
    from pesto_amd import hbonds as H
    g = golden("hbonds")
    s = system(g, "frames")
    x, dh = s["xyz"][:4], np.tile(s["dh"], (4, 1))
    assert dh.shape[0] > SCAN_BLOCK
    xyz = dev(x) if on_device else x
    want_t, want_n = occupancy_def(x, dh, s["acc"], 0.25)
    trip, n = H.baker_hubbard(xyz, dh, s["acc"], 0.25, return_counts=True)
    assert want_n.size > 0 and want_n.size % 4 == 0 and np.array_equal(host(trip), want_t) and np.array_equal(host(n), want_n)
    off, t, d = H.frame_hbonds(xyz, dh, s["acc"])
    w_off, w_t, w_d = frame_hbonds_def(x, dh, s["acc"])
    assert np.array_equal(host(off), w_off) and np.array_equal(host(t), w_t) and np.array_equal(host(d).view(np.uint32), w_d.view(np.uint32))


def test_indices_outside_the_topology_are_refused():
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    g = golden("hbonds")
    s = system(g, "planted")
    x = np.ascontiguousarray(s["xyz"])
    F, N = x.shape[:2]
    model, lib = _default_model(0), _lib.load()
    dh, acc = np.ascontiguousarray(s["dh"]), np.ascontiguousarray(s["acc"])
    P, A = dh.shape[0], acc.shape[0]
    cap = 64
    off, trip, d, n, sz = np.zeros(F + 1, np.int64), np.zeros((cap, 3), np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.int32), np.zeros(1, np.int64)
    bad_dh, bad_acc = dh.copy(), acc.copy()
    bad_dh[-1, 1], bad_acc[0] = N, -1
    for a, b, what in ((bad_dh, acc, b"dh"), (dh, bad_acc, b"acc")):
        rc = lib.pesto_frame_hbonds(model.handle, F, N, P, A, x.ctypes.data, a.ctypes.data, b.ctypes.data, None, 2.5, 10.0, 0.25, cap, off.ctypes.data,
                                    trip.ctypes.data, d.ctypes.data, sz.ctypes.data, _lib.PTR_HOST, None)
        assert rc == -1 and what in lib.pesto_hbonds_last_error() and b"[0, N)" in lib.pesto_hbonds_last_error()
        rc = lib.pesto_hbond_occupancy(model.handle, F, N, P, A, x.ctypes.data, a.ctypes.data, b.ctypes.data, 2.5, 10.0, 0.25, 0.1, cap, trip.ctypes.data,
                                       n.ctypes.data, sz.ctypes.data, _lib.PTR_HOST, None)
        assert rc == -1 and what in lib.pesto_hbonds_last_error()
    u = unwrap_system(g, "uplanted")
    ux, ub = np.ascontiguousarray(u["xyz"]), np.ascontiguousarray(u["box"])
    perm, moff = np.argsort(u["mol"], kind="stable").astype(np.int32), np.array([0, 2, 6, 10], np.int32)
    perm[3] = 10
    out, image = np.zeros_like(ux), np.zeros((3, 3), np.int32)
    rc = lib.pesto_unwrap_pbc(model.handle, 3, 10, 3, ux.ctypes.data, ub.ctypes.data, perm.ctypes.data, moff.ctypes.data, u["masses"].ctypes.data,
                              out.ctypes.data, image.ctypes.data, _lib.PTR_HOST, None)
    assert rc == -1 and b"[0, N)" in lib.pesto_hbonds_last_error()
    # in range but not a permutation: atom perm[4] twice, atom perm[3] never, whose rows of xyz_out no molecule would write
    perm = np.argsort(u["mol"], kind="stable").astype(np.int32)
    perm[3] = perm[4]
    rc = lib.pesto_unwrap_pbc(model.handle, 3, 10, 3, ux.ctypes.data, ub.ctypes.data, perm.ctypes.data, moff.ctypes.data, u["masses"].ctypes.data,
                              out.ctypes.data, image.ctypes.data, _lib.PTR_HOST, None)
    assert rc == -1 and b"repeated" in lib.pesto_hbonds_last_error() and b"[0, N)" not in lib.pesto_hbonds_last_error()
    perm = np.argsort(u["mol"], kind="stable").astype(np.int32)[::-1].copy()     # any order within a molecule's range is a permutation still
    perm[:] = np.concatenate([perm[8:], perm[4:8], perm[:4]])
    rc = lib.pesto_unwrap_pbc(model.handle, 3, 10, 3, ux.ctypes.data, ub.ctypes.data, perm.ctypes.data, moff.ctypes.data, u["masses"].ctypes.data,
                              out.ctypes.data, image.ctypes.data, _lib.PTR_HOST, None)
    assert rc == 0 and np.array_equal(image, g["uplanted_image"]) and np.array_equal(out.view(np.uint32), g["uplanted_out"].view(np.uint32))
