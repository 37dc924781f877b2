"""GPU tests of pesto_amd.dockq (pesto_dockq.hip) against the NumPy definitions of test_dockq_fixture.py, through host arrays and ROCm
tensors: a seeded sweep over the number of decoys, of native pairs and of backbone atoms at the edges of the wave (64) and of the
workgroup (256) - native pairs, preserved and fnat exactly, irmsd bit for bit against docking.irmsd on the GPU, lrmsd within the bound
tests/test_docking.py allows irmsd against its float64 restatement (max(4 e_ref, 4 eps32 max|value|), the worst share printed), the score
within one float32 unit and the class exactly from the returned values; the hand-worked cases; rigid motions; the recorded systems
against native_contacts over residue_contact_maps; fit_rmsd bit for bit against docking.irmsd and trajectory.rmsd; identical bits from call to call and between the
two sides; and a refused call, which writes nothing."""
import numpy as np
import pytest

from conftest import golden
from test_docking_fixture import DOCKING, system, tolerance, ulp_apart
from test_dockq_fixture import (backbone_def, capri_def, dockq_def, fit_rmsd_def, scores_def, sweep_definition, sweep_system, tiny,
                                tiny_decoys)

pytestmark = pytest.mark.gpu

# (P native pairs, F decoys, |S_R|, |S_L|): every P of {1, 63, 64, 65, 257}, F of {1, 2, 65} and selection size of {3, 255, 256, 257}
SWEEP = [(1, 1, 3, 3), (63, 2, 255, 256), (64, 65, 256, 257), (65, 2, 257, 255), (257, 65, 3, 257), (257, 1, 257, 3)]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def bound(value64):
    """the bound of an RMSD against its float64 value: tests/test_docking.py's for irmsd, max(4 e_ref, 4 eps32 max|value|)"""
    return tolerance(golden("docking"), "iface_irmsd", value64)


def check_outputs(out, on_device, F):
    kinds = dict(fnat=np.float32, preserved=np.int32, irmsd=np.float32, lrmsd=np.float32, dockq=np.float32, capri=np.uint8)
    for key, dt in kinds.items():
        v = getattr(out, key)
        assert (v.is_cuda if on_device else isinstance(v, np.ndarray)) and host(v).dtype == dt and host(v).shape == (F,), key
    assert isinstance(out.n_native, int)


def check_against_definition(out, want, tag):
    """the asserts of the sweep on one result; returns the share of the lrmsd bound used"""
    P = want["pairs"].shape[0]
    assert out.n_native == P and np.array_equal(host(out.preserved), want["preserved"]), tag
    assert np.array_equal(host(out.fnat).view(np.uint32), want["fnat"].view(np.uint32)), tag
    tol = bound(want["lrmsd"])
    err = float(np.max(np.abs(host(out.lrmsd).astype(np.float64) - want["lrmsd"])))
    tol_i = bound(want["irmsd"])
    err_i = float(np.max(np.abs(host(out.irmsd).astype(np.float64) - want["irmsd"])))
    print(f"{tag}: lrmsd max deviation {err:.3e}, bound {tol:.3e}, share {err / tol:.3f}; irmsd {err_i:.3e} of {tol_i:.3e}")
    assert err <= tol and err_i <= tol_i, (tag, err, tol, err_i, tol_i)
    score = dockq_def(host(out.fnat), host(out.irmsd), host(out.lrmsd))
    assert ulp_apart(host(out.dockq), score) <= 1, tag
    assert np.array_equal(host(out.capri), capri_def(host(out.preserved), P, host(out.irmsd), host(out.lrmsd))), tag
    return err / tol


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "P%d-F%d-R%d-L%d" % c)
def test_seeded_sweep(case, on_device):
    from pesto_amd import docking as D
    from pesto_amd import dockq as Q
    s, want = sweep_system(*case), sweep_definition(*case)
    P, F, n_SR, n_SL = case
    S_R, S_L = backbone_def(s["ids_R"], s["ids_L"], s["bb"])
    assert want["pairs"].shape[0] == P and S_R.size == n_SR and S_L.size == n_SL and np.bincount(s["roa"]).max() == 70
    xyz = dev(s["xyz"]) if on_device else s["xyz"]
    args = (s["ids_R"], s["ids_L"], s["roa"])
    out = Q.dockq(xyz[:1], xyz, *args, s["bb"])
    check_outputs(out, on_device, F)
    pairs = Q.native_pairs(xyz[0], *args)
    assert (pairs.is_cuda if on_device else isinstance(pairs, np.ndarray)) and host(pairs).dtype == np.int32
    assert np.array_equal(host(pairs), want["pairs"])
    check_against_definition(out, want, "P%d-F%d-R%d-L%d" % case)
    assert same_bits(out.irmsd, D.irmsd(xyz[:1], xyz, *args, ca=s["bb"]))
    # decoy 0 is the reference: (1, 0, 0, 1.0, class 3), exactly
    first = [host(v)[0] for v in (out.fnat, out.irmsd, out.lrmsd, out.dockq, out.capri)]
    assert first == [1.0, 0.0, 0.0, 1.0, 3] and host(out.preserved)[0] == P
    if F == 65:                                         # the decoys run from the bound pose to almost none of it, through every class
        assert host(out.preserved).min() < P // 16 and set(host(out.capri).tolist()) == {0, 1, 2, 3} and np.unique(host(out.preserved)).size > 20


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_hand_worked_cases(on_device):
    from pesto_amd import dockq as Q
    c = tiny()
    xyz, _ = tiny_decoys()
    ref = c["xyz0"]
    if on_device:
        xyz, ref = dev(xyz), dev(ref)
    out = Q.dockq(ref, xyz, c["ids_R"], c["ids_L"], c["roa"], c["bb"], scale=1.0)
    check_outputs(out, on_device, 6)
    assert host(Q.native_pairs(ref, c["ids_R"], c["ids_L"], c["roa"], scale=1.0)).tolist() == [[0, 2], [1, 3]] and out.n_native == 2
    kept, fn, ir, lr, dq, cl = (host(v) for v in (out.preserved, out.fnat, out.irmsd, out.lrmsd, out.dockq, out.capri))
    assert kept.tolist() == [2, 2, 0, 1, 2, 0] and fn.tolist() == [1.0, 1.0, 0.0, 0.5, 1.0, 0.0]          # d = r_contact is no contact; a step closer is
    assert (ir[0], lr[0], dq[0], cl[0]) == (0.0, 0.0, 1.0, 3)                                          # the reference: exact zeros
    assert lr[1] == np.float32(1.25) and lr[5] == np.float32(10.0)                                     # |t| scale, the receptor fitted by the identity
    assert lr[2] == np.float32(100.0) and cl[2] == 0 and cl.tolist() == capri_def(kept, 2, ir, lr).tolist()              # out of reach: class 0
    want = scores_def(host(ref)[None], host(xyz), c["ids_R"], c["ids_L"], c["roa"], c["bb"], 5.0, 10.0, 1.0)
    check_against_definition(out, want, "tiny")
    ten = Q.dockq(ref, xyz, c["ids_R"], c["ids_L"], c["roa"], c["bb"], r_contact=50.0, r_interface=100.0, scale=10.0)     # the same poses read as nanometres
    assert host(ten.preserved).tolist() == [2, 2, 0, 1, 2, 0] and host(ten.lrmsd)[1] == np.float32(12.5)
    assert host(Q.lrmsd(ref, xyz, c["ids_R"], c["ids_L"], c["bb"], scale=1.0))[1] == np.float32(1.25)
    # a [1, N, 3] reference, masks for the subunits and an integer mask for the backbone
    m_R, m_L = np.arange(16) < 8, np.arange(16) >= 8
    again = Q.dockq(ref[None], xyz, m_R, m_L, c["roa"], c["bb"].astype(np.uint8), scale=1.0)
    assert all(same_bits(getattr(out, k), getattr(again, k)) for k in ("fnat", "preserved", "irmsd", "lrmsd", "dockq", "capri"))


def test_a_rigid_motion_of_the_whole_complex_changes_nothing():
    """coordinates rounded to 1/256 A, moved by signed axis permutations and dyadic shifts: the moved frames are exact, so every distance
    keeps its bits and the RMSDs of a moved reference are the fits' own rounding"""
    from pesto_amd import dockq as Q
    s = sweep_system(64, 65, 256, 257)
    x = np.round(s["xyz"][::8].astype(np.float64) * 10.0 * 256.0) / 256.0            # angstroms, F = 9, frame 0 the reference
    turn = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], np.float64), np.array([[0, 1, 0], [-1, 0, 0], [0, 0, 1]], np.float64)
    shift = np.array([3.5, -17.25, 40.0]), np.array([-128.0, 0.125, 2.0])
    assert all(np.linalg.det(t) == 1 for t in turn)
    moved = np.concatenate([x @ turn[0] + shift[0], x @ turn[1] + shift[1]]).astype(np.float32)
    x = x.astype(np.float32)
    assert np.array_equal(moved[:9].astype(np.float64), x.astype(np.float64) @ turn[0] + shift[0])        # exact in float32
    args = (s["ids_R"], s["ids_L"], s["roa"], s["bb"])
    plain = Q.dockq(x[0], x, *args, scale=1.0)
    out = Q.dockq(x[0], moved, *args, scale=1.0)
    assert np.array_equal(np.tile(plain.preserved, 2), out.preserved) and plain.preserved[0] == 64 and plain.preserved.min() < 32
    tol = bound(np.zeros(1))
    print(f"moved reference: irmsd {out.irmsd[[0, 9]]}, lrmsd {out.lrmsd[[0, 9]]}, bound {tol:.3e}")
    assert out.irmsd[[0, 9]].max() <= tol and out.lrmsd[[0, 9]].max() <= tol
    for key in ("irmsd", "lrmsd"):                      # the other decoys keep their RMSDs within the bound as well
        v = np.tile(getattr(plain, key), 2).astype(np.float64)
        assert np.abs(getattr(out, key) - v).max() <= bound(v), key


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name", DOCKING)
def test_recorded_systems_against_native_contacts_over_the_full_maps(name, on_device):
    from pesto_amd import dockq as Q
    from pesto_amd import trajectory as T
    g = golden("docking")
    s = system(g, name)
    xyz, xa, xb = (dev(v) if on_device else v for v in (s["xyz"], s["xa"], s["xb"]))
    out = Q.dockq(xyz[:1], xyz, s["ids_a"], s["ids_b"], s["roa"], s["ca"])
    maps = T.residue_contact_maps(xa, xb, s["res_a"], s["res_b"])
    nat = T.native_contacts(maps[:1], maps)
    assert np.array_equal(host(out.preserved), host(nat).astype(np.int32)) and out.n_native == int(host(maps[0]).sum())
    assert out.n_native == int(g[name + "_roff"][1]) and host(out.preserved)[0] == out.n_native
    # with bb = ca the irmsd is the recorded one, within its bound; frame 0 is the reference
    want = g[name + "_irmsd_f64"]
    assert np.abs(host(out.irmsd).astype(np.float64) - want).max() <= tolerance(g, name + "_irmsd", want) and host(out.irmsd)[0] == 0
    S_R, S_L = backbone_def(s["ids_a"], s["ids_b"], s["ca"])
    lr = fit_rmsd_def(s["xyz"][:1], s["xyz"], S_R, S_L)
    assert np.abs(host(out.lrmsd).astype(np.float64) - lr).max() <= bound(lr) and host(out.lrmsd)[0] == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_fit_rmsd(on_device):
    from pesto_amd import docking as D
    from pesto_amd import dockq as Q
    from pesto_amd import trajectory as T
    s = sweep_system(65, 2, 257, 255)
    big = sweep_system(64, 65, 256, 257)
    for z in (s, big):
        xyz = dev(z["xyz"]) if on_device else z["xyz"]
        S_R, S_L = backbone_def(z["ids_R"], z["ids_L"], z["bb"])
        # fit and measure on the same atoms: docking's interface RMSD on that selection (a threshold beyond every distance makes every
        # atom an interface atom, the mask picks S_R) bit for bit, and trajectory.rmsd bit for bit off the reference frame, where the
        # identity short cut gives exactly 0 against trajectory.rmsd's some 1e-15
        both = Q.fit_rmsd(xyz[:1], xyz, S_R, S_R)
        plain = T.rmsd(xyz[:1], xyz, S_R, S_R)
        only_R = np.zeros(z["xyz"].shape[1], bool)
        only_R[S_R] = True
        assert (both.is_cuda if on_device else isinstance(both, np.ndarray)) and host(both).dtype == np.float32
        assert same_bits(both, D.irmsd(xyz[:1], xyz, z["ids_R"], z["ids_L"], z["roa"], only_R, r_thr=1e6))
        assert same_bits(host(both)[1:], host(plain)[1:]) and host(both)[0] == 0
        assert np.abs(host(both).astype(np.float64) - host(plain)).max() <= bound(host(plain))
        want = fit_rmsd_def(z["xyz"][:1], z["xyz"], S_R, S_R)
        assert np.abs(host(both).astype(np.float64) - want).max() <= bound(want)
        # the ligand RMSD is fit_rmsd on S_R and S_L, bit for bit, here and in dockq
        lr = Q.lrmsd(xyz[:1], xyz, z["ids_R"], z["ids_L"], z["bb"])
        assert same_bits(lr, Q.fit_rmsd(xyz[:1], xyz, S_R, S_L))
        assert same_bits(lr, Q.dockq(xyz[:1], xyz, z["ids_R"], z["ids_L"], z["roa"], z["bb"]).lrmsd)
        want = fit_rmsd_def(z["xyz"][:1], z["xyz"], S_R, S_L)
        assert np.abs(host(lr).astype(np.float64) - want).max() <= bound(want)
        # masks select the same atoms; one reference frame per frame gives the same bits; an unsorted measure set is a set
        mask = np.zeros(z["xyz"].shape[1], bool)
        mask[S_L] = True
        F = z["xyz"].shape[0]
        ref_f = np.repeat(z["xyz"][:1], F, 0)
        assert same_bits(lr, Q.fit_rmsd(dev(ref_f) if on_device else ref_f, xyz, S_R, mask))
        other = Q.fit_rmsd(xyz[:1], xyz, S_R, S_L[::-1].copy())
        assert np.abs(host(other).astype(np.float64) - want).max() <= bound(want)


def test_bits_repeat_from_call_to_call_and_between_the_two_sides():
    from pesto_amd import dockq as Q
    s = sweep_system(64, 65, 256, 257)
    args = (s["ids_R"], s["ids_L"], s["roa"], s["bb"])
    keys = ("fnat", "preserved", "irmsd", "lrmsd", "dockq", "capri")
    a = Q.dockq(s["xyz"][:1], s["xyz"], *args)
    b = Q.dockq(s["xyz"][:1], s["xyz"], *args)
    d = dev(s["xyz"])
    c = Q.dockq(d[:1], d, *args)
    e = Q.dockq(s["xyz"][0], d, *(dev(v) for v in args))             # a host reference, everything else on the device
    for other in (b, c, e):
        assert all(same_bits(getattr(a, k), getattr(other, k)) for k in keys) and other.n_native == a.n_native
    assert c.fnat.is_cuda and e.capri.is_cuda
    assert same_bits(Q.lrmsd(s["xyz"][:1], s["xyz"], *args[:2], s["bb"]), Q.lrmsd(d[:1], d, *args[:2], s["bb"]))
    assert same_bits(Q.native_pairs(s["xyz"][0], *args[:3]), Q.native_pairs(d[0], *args[:3]))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_refused_call_writes_nothing(on_device):
    from pesto_amd import _lib
    from pesto_amd import dockq as Q
    from pesto_amd.patches import _default_model
    c = tiny()
    xyz, _ = tiny_decoys()
    F, N = xyz.shape[:2]
    model, lib = _default_model(0), _lib.load()
    pairs, ranges, perm = Q._native(c["xyz0"][None], c["ids_R"].astype(np.int32), c["ids_L"].astype(np.int32), c["roa"], 5.0, 1.0, model)
    good = dict(ranges=ranges, perm=perm, sel_I=np.array([0, 1, 2, 8, 9, 10], np.int32), sel_R=np.array([0, 1, 2, 4, 5, 6], np.int32),
                sel_L=np.array([8, 9, 10], np.int32))
    place = (lambda a: dev(a)) if on_device else (lambda a: np.ascontiguousarray(a))
    side = _lib.Side(place(xyz), model._gpu)
    kinds = (np.float32, np.int32, np.float32, np.float32, np.float32, np.uint8)

    def call(**bad):
        v = {k: place(a) for k, a in dict(good, **bad).items()}
        outs = [place(np.full(F, 7, dt)) for dt in kinds]
        x, y = place(xyz), place(c["xyz0"])
        rc = lib.pesto_dockq(model.handle, F, N, side.ptr(y), side.ptr(x), v["ranges"].shape[0], side.ptr(v["ranges"]), v["perm"].shape[0],
                             side.ptr(v["perm"]), v["sel_I"].shape[0], side.ptr(v["sel_I"]), v["sel_R"].shape[0], side.ptr(v["sel_R"]),
                             v["sel_L"].shape[0], side.ptr(v["sel_L"]), 5.0, 1.0, *(side.ptr(o) for o in outs), side.kind, side.stream)
        return rc, [host(o) for o in outs]

    rc, outs = call()
    assert rc == 0 and outs[1].tolist() == [2, 2, 0, 1, 2, 0] and outs[5][0] == 3 and outs[3][1] == np.float32(1.25)
    over = lambda a, k, v: np.concatenate([a[:k], [v], a[k + 1:]]).astype(np.int32)
    for bad in (dict(sel_I=over(good["sel_I"], 5, N)), dict(sel_R=over(good["sel_R"], 0, N)), dict(sel_L=over(good["sel_L"], 2, N + 7)),
                dict(sel_L=over(good["sel_L"], 0, -1)), dict(perm=over(perm, 15, N))):
        rc, outs = call(**bad)
        assert rc == -1 and b"[0, N)" in lib.pesto_dockq_last_error(), bad
        assert all((o == 7).all() for o in outs), bad
    for k, col, v in ((0, 1, 0), (1, 3, 17), (0, 2, -1), (1, 0, 9)):            # an empty range, one past the permutation, a negative start, a reversed one
        r = ranges.copy()
        r[k, col] = v
        rc, outs = call(ranges=r)
        assert rc == -1 and b"ranges" in lib.pesto_dockq_last_error() and all((o == 7).all() for o in outs), (k, col, v)
    # pesto_fit_rmsd likewise
    out = place(np.full(F, 7, np.float32))
    x, y = place(xyz), place(c["xyz0"])
    for sf, sm in ((over(good["sel_R"], 3, N), good["sel_L"]), (good["sel_R"], over(good["sel_L"], 1, N))):
        sf, sm = place(sf), place(sm)
        rc = lib.pesto_fit_rmsd(model.handle, F, 1, N, side.ptr(y), side.ptr(x), 6, side.ptr(sf), 3, side.ptr(sm), 1.0, side.ptr(out), side.kind, side.stream)
        assert rc == -1 and b"[0, N)" in lib.pesto_dockq_last_error() and (host(out) == 7).all()
    # what the host refuses before any launch
    sf, sm = place(good["sel_R"]), place(good["sel_L"])
    assert lib.pesto_fit_rmsd(model.handle, F, 1, N, side.ptr(y), side.ptr(x), 2, side.ptr(sf), 3, side.ptr(sm), 1.0, side.ptr(out), side.kind, side.stream) == -1
    assert lib.pesto_fit_rmsd(model.handle, F, 2, N, side.ptr(y), side.ptr(x), 6, side.ptr(sf), 3, side.ptr(sm), 1.0, side.ptr(out), side.kind, side.stream) == -1
    assert (host(out) == 7).all()
