"""GPU tests of pesto_amd.docking (pesto_docking.hip) against the definitions the reference's trajectory_utils functions were checked
against when tests/golden/docking.npz was made (tests/test_docking_fixture.py holds the NumPy restatements): frame contact lists, residue
pairs and interface atoms exactly and d / dmin bit for bit, through host arrays and ROCm tensors, with the capacity protocol and identical
bits from call to call; irmsd, t and r within max(4 e_ref, 4 eps32 max|value|) of the float64 restatement, exactly 0 for the frame that is
its reference; Model.forward_frames followed by interface_atoms and irmsd on the same ROCm tensor."""
import numpy as np
import pytest

from conftest import golden, md_frames, weights
from test_docking_fixture import DOCKING, SYSTEMS, contacts_def, docking64, interface_def, irmsd64, system, tolerance

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


def check_lists(g, name, got, keys=("off", "pairs", "d"), on_device=False):
    off, rows, val = got
    assert (off.is_cuda and rows.is_cuda and val.is_cuda) if on_device else all(isinstance(v, np.ndarray) for v in got)
    assert host(off).dtype == np.int64 and host(rows).dtype == np.int32 and host(val).dtype == np.float32
    assert np.array_equal(host(off), g[f"{name}_{keys[0]}"]), name
    assert host(rows).shape == g[f"{name}_{keys[1]}"].shape and np.array_equal(host(rows), g[f"{name}_{keys[1]}"].astype(np.int32)), name
    assert np.array_equal(host(val).view(np.uint32), g[f"{name}_{keys[2]}"].view(np.uint32)), name


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_frame_contacts_and_contacts(name, on_device):
    from pesto_amd import docking as D
    g = golden("docking")
    s = system(g, name)
    xa, xb = place(on_device, s["xa"], s["xb"])
    got = D.frame_contacts(xa, xb)
    check_lists(g, name, got, on_device=on_device)
    again = D.frame_contacts(xa, xb)
    assert all(same_bits(u, v) for u, v in zip(got, again))
    # the reference's form, mapped through the subunits' atom indices
    off, pairs, d = g[name + "_off"], g[name + "_pairs"].astype(np.int64), g[name + "_d"]
    frames = D.contacts(xa, xb, s["ids_a"], s["ids_b"])
    assert len(frames) == off.size - 1
    for f, (df, ids) in enumerate(frames):
        p = pairs[off[f]:off[f + 1]]
        assert host(ids).dtype == np.int32 and np.array_equal(host(ids), np.stack([s["ids_a"][p[:, 0]], s["ids_b"][p[:, 1]]], 1))
        assert np.array_equal(host(df).view(np.uint32), d[off[f]:off[f + 1]].view(np.uint32))
    if name == "iface":
        assert np.array_equal(host(D.frame_contacts(xa, xb, r_thr=4.1)[0]), g["iface_off41"])
        if not on_device:                               # angstroms with scale 1, against the definition evaluated here
            ang = (g["iface_xyz256"].astype(np.float64) / 256.0).astype(np.float32)[:8]
            aa, ab = np.ascontiguousarray(ang[:, s["ids_a"]]), np.ascontiguousarray(ang[:, s["ids_b"]])
            o, p, dd = D.frame_contacts(aa, ab, 5.0, 1.0)
            wo, wp, wd = contacts_def(aa, ab, 5.0, 1.0)
            assert np.array_equal(o, wo) and np.array_equal(o, g["iface_off_angstrom"][:9]) and np.array_equal(p, wp)
            assert np.array_equal(dd.view(np.uint32), wd.view(np.uint32))
    if name == "single":                                # a single frame [N, 3]
        o, p, dd = D.frame_contacts(xa[0], xb[0])
        assert host(o).tolist() == [0, 1] and host(p).tolist() == [[0, 0]] and host(dd).tolist() == [0.0]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_capacity_too_small_returns_the_count_and_the_repeat_completes(on_device):
    from pesto_amd import _lib
    from pesto_amd import docking as D
    from pesto_amd.patches import _default_model
    g = golden("docking")
    s = system(g, "size")
    xa, xb = place(on_device, s["xa"], s["xb"])
    F, Na, Nb = s["xa"].shape[0], s["xa"].shape[1], s["xb"].shape[1]
    K = int(g["size_off"][-1])
    model = _default_model(0)
    side = _lib.Side(xa, model._gpu)
    lib = _lib.load()
    for cap in (16, K - 1, K):
        off, pairs, d, sz = side.empty((F + 1,), np.int64), side.empty((cap, 2), np.int32), side.empty((cap,), np.float32), np.zeros(1, np.int64)
        _lib.check(lib.pesto_frame_contacts(model.handle, F, Na, Nb, side.ptr(xa), side.ptr(xb), 5.0, 10.0, cap, side.ptr(off), side.ptr(pairs),
                                            side.ptr(d), sz.ctypes.data, side.kind, side.stream), lib.pesto_docking_last_error)
        assert int(sz[0]) == K and np.array_equal(host(off), g["size_off"]), cap            # the count and the offsets come back either way
        if cap == K:
            check_lists(g, "size", (off, pairs, d), on_device=on_device)
    check_lists(g, "size", D.frame_contacts(xa, xb, capacity=16), on_device=on_device)
    check_lists(g, "size", D.frame_contacts(xa, xb, capacity=K), on_device=on_device)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_frame_residue_contacts(name, on_device):
    from pesto_amd import docking as D
    g = golden("docking")
    s = system(g, name)
    xa, xb, ra, rb = place(on_device, s["xa"], s["xb"], s["res_a"], s["res_b"])
    got = D.frame_residue_contacts(xa, xb, ra, rb)
    check_lists(g, name, got, ("roff", "rpairs", "dmin"), on_device)
    fed = D.frame_residue_contacts(D.frame_contacts(xa, xb), res_a=ra, res_b=rb)
    assert all(same_bits(u, v) for u, v in zip(got, fed))
    # the recorded lists fed in from the other side of the call
    lists = place(not on_device, g[name + "_off"], g[name + "_pairs"].astype(np.int32), g[name + "_d"])
    check_lists(g, name, D.frame_residue_contacts(tuple(lists), res_a=s["res_a"], res_b=s["res_b"]), ("roff", "rpairs", "dmin"), not on_device)
    if name == "planted":                               # an atom index or a residue row outside its range is refused
        bad = g[name + "_pairs"].astype(np.int32)
        bad[0, 1] = s["xb"].shape[1]
        from pesto_amd._lib import PestoError
        with pytest.raises(PestoError):
            D.frame_residue_contacts((g[name + "_off"], bad, g[name + "_d"]), res_a=s["res_a"], res_b=s["res_b"])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", SYSTEMS)
def test_interface_atoms(name, on_device):
    from pesto_amd import docking as D
    g = golden("docking")
    s = system(g, name)
    (xyz,) = place(on_device, s["xyz"])
    for x0 in (xyz, xyz[0]):                            # frame 0 of a trajectory, or the frame itself
        ira, irb = D.interface_atoms(x0, s["ids_a"], s["ids_b"], s["roa"])
        assert (ira.is_cuda and irb.is_cuda) if on_device else (isinstance(ira, np.ndarray) and isinstance(irb, np.ndarray))
        assert host(ira).dtype == np.int64 and host(irb).dtype == np.int64
        assert np.array_equal(host(ira), g[name + "_ira"]) and np.array_equal(host(irb), g[name + "_irb"]), name
    if name == "iface":                                 # another threshold, against the definition evaluated here
        ira, irb = D.interface_atoms(xyz, s["ids_a"], s["ids_b"], s["roa"], r_thr=4.1)
        wa, wb = interface_def(s["xyz"][0], s["ids_a"], s["ids_b"], s["roa"], 4.1)
        assert np.array_equal(host(ira), wa) and np.array_equal(host(irb), wb) and 0 < wa.size < g["iface_ira"].size


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", DOCKING)
def test_irmsd_and_rigid_docking(name, on_device):
    from pesto_amd import docking as D
    g = golden("docking")
    s = system(g, name)
    (xyz,) = place(on_device, s["xyz"])
    args = (s["ids_a"], s["ids_b"], s["roa"])
    rm = D.irmsd(xyz[:1], xyz, *args, s["ca"])
    t, r = D.interface_rigid_docking(xyz[:1], xyz, *args)
    F = s["xyz"].shape[0]
    for key, got in (("irmsd", rm), ("t", t), ("r", r)):
        assert (got.is_cuda if on_device else isinstance(got, np.ndarray)) and host(got).dtype == np.float32
        want = g[f"{name}_{key}_f64"]
        assert host(got).shape == want.shape == ((F,) if key == "irmsd" else (F, 3))
        tol = tolerance(g, f"{name}_{key}", want)
        err = float(np.max(np.abs(host(got).astype(np.float64) - want)))
        print(f"{name}_{key}: max deviation {err:.3e}, bound {tol:.3e}")
        assert err <= tol, (key, err, tol)
    # the yardstick evaluated here agrees with the recorded one
    assert np.allclose(irmsd64(s["xyz"][:1], s["xyz"], *args, s["ca"])[0], g[name + "_irmsd_f64"], rtol=1e-9, atol=1e-11)
    assert np.allclose(docking64(s["xyz"][:1], s["xyz"], *args)[1], g[name + "_r_f64"], rtol=1e-9, atol=1e-11)
    # identical bits from run to run, between the two sides of the call, and with one reference frame per frame
    rm2 = D.irmsd(xyz[:1], xyz, *args, s["ca"])
    t2, r2 = D.interface_rigid_docking(xyz[:1], xyz, *args)
    assert same_bits(rm, rm2) and same_bits(t, t2) and same_bits(r, r2)
    (other,) = place(not on_device, s["xyz"])
    to, ro = D.interface_rigid_docking(other[:1], other, *args)
    assert same_bits(t, to) and same_bits(r, ro) and same_bits(rm, D.irmsd(other[:1], other, *args, s["ca"]))
    ref_f = np.repeat(s["xyz"][:1], F, 0)
    (ref_f,) = place(on_device, ref_f)
    tf, rf = D.interface_rigid_docking(ref_f, xyz, *args)
    assert same_bits(t, tf) and same_bits(r, rf) and same_bits(rm, D.irmsd(ref_f, xyz, *args, s["ca"]))
    # irmsd is trajectory.rmsd on the interface's CA atoms, bit for bit, but for the frame that is its reference: exactly 0 there
    from pesto_amd import trajectory as T
    sel = irmsd64(s["xyz"][:1], s["xyz"], *args, s["ca"])[1]
    plain = host(T.rmsd(xyz[:1], xyz, sel, sel))
    print(f"{name}: irmsd of the reference itself {float(host(rm)[0]):.3e}, trajectory.rmsd {float(plain[0]):.3e}")
    assert host(rm)[0] == 0 and plain[0] < 1e-12 and same_bits(host(rm)[1:], plain[1:])
    if name == "rigid":                                 # frame 0 is the reference itself: exactly 0
        assert not host(t)[0].any() and not host(r)[0].any()
        assert np.abs(host(r)[1:]).max() > 0.1 and np.abs(host(t)[1:]).max() > 0.1


def test_forward_frames_then_interface_and_irmsd_on_the_device():
    import torch
    from pesto_amd import Model
    from pesto_amd import docking as D
    from pesto_amd.config import CONFIGS
    f = md_frames()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    roa = dev(f["res_of_atom"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), roa.long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    assert z.is_cuda and np.abs(host(z) - f["z"]).max() < 1e-4
    # the molecule's two halves stand for two subunits, the second atom of every residue for its CA; the coordinates are angstroms
    roa_h = f["res_of_atom"].astype(np.int64)
    ids_a, ids_b = np.nonzero(roa_h < f["R"] // 2)[0], np.nonzero(roa_h >= f["R"] // 2)[0]
    ca = np.zeros(roa_h.size, bool)
    ca[np.unique(roa_h, return_index=True)[1] + 1] = True
    ira, irb = D.interface_atoms(X, ids_a, ids_b, roa, scale=1.0, model=m)
    rm = D.irmsd(X[:1], X, ids_a, ids_b, roa, ca, scale=1.0, model=m)
    t, r = D.interface_rigid_docking(X[:1], X, ids_a, ids_b, roa, scale=1.0, model=m)
    assert ira.is_cuda and irb.is_cuda and rm.is_cuda and t.is_cuda and r.is_cuda
    wa, wb = interface_def(f["X_frames"][0], ids_a, ids_b, roa_h, 10.0, 1.0)
    assert np.array_equal(host(ira), wa) and np.array_equal(host(irb), wb) and wa.size >= 3 and wb.size >= 3
    # double evaluation rounded once: within 4 eps32 of the largest value
    want, sel = irmsd64(f["X_frames"][:1], f["X_frames"], ids_a, ids_b, roa_h, ca, 10.0, 1.0)
    assert sel.size >= 3 and np.abs(host(rm) - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()
    t64, r64, _ = docking64(f["X_frames"][:1], f["X_frames"], ids_a, ids_b, roa_h, 10.0, 1.0)
    assert np.linalg.norm(r64, axis=1).max() < 2.5
    assert np.abs(host(t) - t64).max() <= 4 * np.finfo(np.float32).eps * np.abs(t64).max()
    assert np.abs(host(r) - r64).max() <= 4 * np.finfo(np.float32).eps * np.abs(r64).max()
    # the same through host arrays; frame 0 is the reference itself
    assert same_bits(rm, D.irmsd(f["X_frames"][:1], f["X_frames"], ids_a, ids_b, roa_h, ca, scale=1.0))
    th, rh = D.interface_rigid_docking(f["X_frames"][:1], f["X_frames"], ids_a, ids_b, roa_h, scale=1.0)
    assert same_bits(t, th) and same_bits(r, rh) and not host(t)[0].any() and not host(r)[0].any() and host(rm)[0] == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_more_frames_than_the_offsets_scan_has_threads(on_device):
    """1,200 frames (the planted frames and an empty one in turn): every thread of the one workgroup that scans the frames' totals owns
    two frames, and the residue pairs go through the same scan"""
    from pesto_amd import docking as D
    g = golden("docking")
    s = system(g, "e1")
    xa, xb = np.tile(s["xa"], (400, 1, 1)), np.tile(s["xb"], (400, 1, 1))
    want = contacts_def(xa, xb)
    assert want[0].size == 1201 and want[0][-1] == 400 * g["e1_off"][-1]
    da, db = place(on_device, xa, xb)
    got = D.frame_contacts(da, db)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1])
    assert np.array_equal(host(got[2]).view(np.uint32), want[2].view(np.uint32))
    roff, rpairs, dmin = D.frame_residue_contacts(got, res_a=s["res_a"], res_b=s["res_b"])
    U = int(g["e1_roff"][-1])
    assert np.array_equal(host(roff), np.concatenate([[0], (g["e1_roff"][1:][None] + U * np.arange(400)[:, None]).reshape(-1)]))
    assert np.array_equal(host(rpairs), np.tile(g["e1_rpairs"].astype(np.int32), (400, 1)))
    assert np.array_equal(host(dmin).view(np.uint32), np.tile(g["e1_dmin"], 400).view(np.uint32))


def test_selection_indices_outside_the_topology_are_refused():
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    g = golden("docking")
    x = np.ascontiguousarray(system(g, "rigid")["xyz"])
    F, N = x.shape[:2]
    model, lib = _default_model(0), _lib.load()
    ok, bad = np.arange(24, dtype=np.int32), np.array([0, 1, N], np.int32)
    t, r, rm = np.zeros((F, 3), np.float32), np.zeros((F, 3), np.float32), np.zeros(F, np.float32)
    for sel_r, sel_l in ((bad, ok), (ok, bad)):
        rc = lib.pesto_rigid_docking(model.handle, F, 1, N, x.ctypes.data, x.ctypes.data, sel_r.size, sel_r.ctypes.data, sel_l.size, sel_l.ctypes.data,
                                     t.ctypes.data, r.ctypes.data, _lib.PTR_HOST, None)
        assert rc == -1 and b"[0, N)" in lib.pesto_docking_last_error()
    rc = lib.pesto_interface_rmsd(model.handle, F, 1, N, x.ctypes.data, x.ctypes.data, bad.size, bad.ctypes.data, 10.0, rm.ctypes.data, _lib.PTR_HOST, None)
    assert rc == -1 and b"[0, N)" in lib.pesto_docking_last_error()
