"""GPU sweeps of the analysis entry points over the seeded cases of tests/analysis_sweep.py (their generators are checked without a GPU by
tests/test_analysis_sweep_fixture.py): pesto_amd.trajectory, docking, hbonds, sasa and the two cell-grid contact searches against the
definitions the fixture modules hold, at the tile edges of the kernels' constants, with lattice coordinates whose thresholds and bin edges
are attained exactly, rough coordinates out to PDB's range, NaN and infinite coordinates, and the superposition families through all three
users of kabsch_rotation.

What is exact: counts, P, contact maps, native contacts, fnat; hbond lists, d, occupancy lists, unwrapped coordinates and images; docking
lists, d, residue pairs, dmin, interface atoms; SASA counts, areas and residue sums; cell-grid pairs, d (the float32 fma chain), tie flags
and labels. What has a tolerance, and the rule it comes from: L, KL, centroids, t, t_ref, R, superposed coordinates, the rigid docking's t
and r within 4 eps32 max|value| of the float64 restatement (the groups' rule where no reference deviation is recorded); rmsd and irmsd
within 4 eps32 max(max|value|, max|xyz|) (test_degenerate_selection_gives_a_finite_proper_rotation's rule).

Every case runs from ROCm tensors; every third case of a list from host arrays too, with identical bytes. The list entry points run once
more with a capacity one below the true count."""
import math

import numpy as np
import pytest

import analysis_sweep as S
from test_cellgrid import _run as run_cellgrid

pytestmark = pytest.mark.gpu
EPS32 = S.EPS32


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def place(on_device, *arrays):
    return [dev(a) if on_device else a for a in arrays]


def sides(entry, case):
    return [True, False] if S.every_third(entry, case) else [True]


def exact(case, what, got, want):
    """identical dtype, shape and bytes (NaN payloads included), or a message with the case tuple and the first differing index"""
    got, want = np.ascontiguousarray(host(got)), np.ascontiguousarray(np.asarray(want))
    if got.dtype.kind in "iu" and want.dtype.kind in "iu" and got.dtype.itemsize == want.dtype.itemsize:
        got = got.view(want.dtype)                      # (uint32 outputs come back from the device as the int32 of the same bits)
    assert got.dtype == want.dtype and got.shape == want.shape, (case, what, got.dtype, got.shape, want.dtype, want.shape)
    if got.tobytes() != want.tobytes():
        diff = np.nonzero(got.reshape(-1).view(np.uint8).reshape(got.size, -1) != want.reshape(-1).view(np.uint8).reshape(want.size, -1))[0]
        k = np.unravel_index(int(diff[0]), got.shape) if got.shape else ()
        raise AssertionError(f"{case}: {what} differs first at index {k}: got {got[k]!r}, want {want[k]!r} ({np.unique(diff).size} of {got.size} entries differ)")


def close(case, what, got, want64, bound):
    """|got - want64| <= bound, NaN where and only where want64 has one"""
    got = host(got).astype(np.float64)
    want64 = np.asarray(want64, np.float64)
    assert got.shape == want64.shape, (case, what, got.shape, want64.shape)
    assert np.array_equal(np.isnan(got), np.isnan(want64)), (case, what, "NaN pattern")
    err = np.where(np.isnan(want64), 0.0, np.abs(got - want64))
    worst = float(err.max()) if err.size else 0.0
    print(f"{S.case_id(case)} {what}: max deviation {worst:.3e}, bound {bound:.3e}")
    if worst > bound:
        k = np.unravel_index(int(np.argmax(err > bound)), err.shape)
        raise AssertionError(f"{case}: {what} off by {worst:.3e} > {bound:.3e}, first at index {k}: got {got[k]!r}, want {want64[k]!r}")


def bound4(want64):
    v = np.abs(np.asarray(want64, np.float64))
    return 4.0 * EPS32 * float(np.nanmax(v)) if v.size else 0.0


def same_bytes(case, a, b):
    """the outputs of the device run and of the host run of a case"""
    assert a.keys() == b.keys()
    for k in a:
        exact(case, f"host against device: {k}", b[k], host(a[k]))


# ================================================================== pesto_amd.trajectory
@pytest.mark.parametrize("case", S.COUNTS, ids=S.case_id)
def test_contact_counts_and_distribution(case):
    from pesto_amd import trajectory as T
    c = S.build("counts", case)
    runs = []
    for on_device in sides("counts", case):
        a, b = place(on_device, c["x0"], c["x1"])
        out = {}
        for tag, splits in (("", c["frame_splits"]), ("_default", None), ("_one", 1)):
            out["counts" + tag] = host(T.contact_counts(a, b, bins=c["bins"], frame_splits=splits))
            out["P" + tag] = host(T.contacts_distribution(a, a if b is None else b, c["bins"], frame_splits=splits))
            exact(case, "counts" + tag, out["counts" + tag], c["counts"])
            exact(case, "P" + tag, out["P" + tag], c["P"])
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


@pytest.mark.parametrize("case", S.LOGLIK, ids=S.case_id)
def test_loglikelihood_and_div_kl(case):
    from pesto_amd import trajectory as T
    c = S.build("loglik", case)
    runs = []
    for on_device in sides("loglik", case):
        a, b, y0, y1, p, q = place(on_device, c["x0"], c["x1"], c["y0"], c["y1"], c["P"], c["Q"])
        m = T.StatisticalContactsModel(0.0, 1.0, 2)
        m.bins = c["bins"]
        m.fit(a, b)
        exact(case, "fitted P", m.P, c["P"])
        out = dict(L=host(m.loglikelihood(a, b)), L_other=host(m.loglikelihood(y0, y1)), KL=host(T.div_KL(q, p)))
        for k in out:
            assert out[k].dtype == np.float32
            close(case, k, out[k], c[k], bound4(c[k]))
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


@pytest.mark.parametrize("case", S.MAPS, ids=S.case_id)
def test_contact_maps_native_contacts_and_fnat(case):
    from pesto_amd import trajectory as T
    c = S.build("maps", case)
    runs = []
    for on_device in sides("maps", case):
        a, b = place(on_device, c["xa"], c["xb"])
        m = T.residue_contact_maps(a, b, c["res_a"], c["res_b"], r_thr=c["r_thr"], scale=c["scale"])
        out = dict(maps=host(m), native=host(T.native_contacts(m[:1], m)), fnat=host(T.fnat(m[:1], m)))
        for k in out:
            exact(case, k, out[k], c[k])
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


@pytest.mark.parametrize("case", S.CENTROIDS, ids=S.case_id)
def test_residue_centroids(case):
    from pesto_amd import trajectory as T
    c = S.build("centroids", case)
    runs = []
    for on_device in sides("centroids", case):
        x, r = place(on_device, c["x"], c["roa"])
        out = dict(centroids=host(T.residue_centroids(x, r, c["R"])))
        close(case, "centroids", out["centroids"], c["want"], bound4(c["want"]))
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


# ================================================================== pesto_amd.hbonds
def hbond_lists_with_a_small_capacity(case, c, on_device):
    """pesto_frame_hbonds and pesto_hbond_occupancy with room for one entry less than there are: the count and the offsets come back,
    nothing is written behind the capacity; then the Python call, which repeats with the count"""
    from pesto_amd import _lib
    from pesto_amd import hbonds as H
    from pesto_amd.patches import _default_model
    F, N = c["xyz"].shape[:2]
    P, A = c["dh"].shape[0], c["acc"].shape[0]
    K, k = int(c["off"][-1]), int(c["occ_n"].size)
    model, lib = _default_model(0), _lib.load()
    (xyz,) = place(on_device, c["xyz"])
    side = _lib.Side(xyz, model._gpu)
    dh, acc = side.put(c["dh"], np.int32), side.put(c["acc"], np.int32)
    k2 = math.cos(math.radians(c["angle"])) ** 2
    if K >= 2:
        cap = K - 1
        off, trip, d, sz = side.empty((F + 1,), np.int64), side.empty((cap + 8, 3), np.int32), side.empty((cap + 8,), np.float32), np.zeros(1, np.int64)
        trip[cap:], d[cap:] = -7, -7.0
        _lib.check(lib.pesto_frame_hbonds(model.handle, F, N, P, A, side.ptr(xyz), side.ptr(dh), side.ptr(acc), None, c["r_thr"], c["scale"], float(k2),
                                          cap, side.ptr(off), side.ptr(trip), side.ptr(d), sz.ctypes.data, side.kind, side.stream), lib.pesto_hbonds_last_error)
        assert int(sz[0]) == K, (case, int(sz[0]), K)
        exact(case, "offsets at capacity K - 1", off, c["off"])
        assert np.all(host(trip)[cap:] == -7) and np.all(host(d)[cap:] == -7.0), case
        got = H.frame_hbonds(xyz, c["dh"], c["acc"], c["r_thr"], c["angle"], c["scale"], capacity=cap)
        for name, g, w in zip(("offsets", "triplets", "d"), got, (c["off"], c["trip"], c["d"])):
            exact(case, f"{name} after the repeat", g, w)
    if k >= 2:
        cap = k - 1
        trip, n, sz = side.empty((cap + 8, 3), np.int32), side.empty((cap + 8,), np.int32), np.zeros(1, np.int64)
        trip[cap:], n[cap:] = -7, -7
        _lib.check(lib.pesto_hbond_occupancy(model.handle, F, N, P, A, side.ptr(xyz), side.ptr(dh), side.ptr(acc), c["r_thr"], c["scale"], float(k2),
                                             c["freq"], cap, side.ptr(trip), side.ptr(n), sz.ctypes.data, side.kind, side.stream),
                   lib.pesto_hbonds_last_error)
        assert int(sz[0]) == k and np.all(host(trip)[cap:] == -7) and np.all(host(n)[cap:] == -7), (case, int(sz[0]), k)


@pytest.mark.parametrize("case", S.HBONDS, ids=S.case_id)
def test_hbond_lists_occupancy_and_subunit_bonds(case):
    from pesto_amd import hbonds as H
    c = S.build("hbonds", case)
    crit = dict(r_thr=c["r_thr"], angle=c["angle"], scale=c["scale"])
    runs = []
    for on_device in sides("hbonds", case):
        (xyz,) = place(on_device, c["xyz"])
        out = {}
        out["off"], out["trip"], out["d"] = (host(v) for v in H.frame_hbonds(xyz, c["dh"], c["acc"], **crit))
        out["occ_trip"], out["occ_n"] = (host(v) for v in H.baker_hubbard(xyz, c["dh"], c["acc"], c["freq"], return_counts=True, **crit))
        if c["group"] is not None:
            (grp,) = place(on_device, c["group"])
            out["goff"], out["gtrip"], out["gd"] = (host(v) for v in H.frame_hbonds(xyz, c["dh"], c["acc"], group=grp, **crit))
            nhb, rows = H.hydrogen_bonds(xyz, c["dh"], c["acc"], np.nonzero(c["group"] == 1)[0], np.nonzero(c["group"] == 2)[0], **crit)
            out["nhb"] = host(nhb)
            out["rows"] = np.concatenate([host(r) for r in rows]).reshape(-1, 3)
            assert len(rows) == c["nhb"].size and [int(r.shape[0]) for r in rows] == c["nhb"].astype(np.int64).tolist(), case
        for k in out:
            exact(case, k, out[k], c[k])
        hbond_lists_with_a_small_capacity(case, c, on_device)
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


@pytest.mark.parametrize("case", S.UNWRAP, ids=S.case_id)
def test_unwrap_pbc(case):
    from pesto_amd import hbonds as H
    c = S.build("unwrap", case)
    runs = []
    for on_device in sides("unwrap", case):
        xyz, box = place(on_device, c["xyz"], c["box"])
        before = host(xyz).copy()
        got, image = H.unwrap_pbc(xyz, box, c["mol"], c["masses"], return_images=True)
        out = dict(out=host(got), image=host(image))
        for k in out:
            exact(case, k, out[k], c[k])
        exact(case, "the input", xyz, before)
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


# ================================================================== pesto_amd.docking
def contact_lists_with_a_small_capacity(case, c, on_device):
    from pesto_amd import _lib
    from pesto_amd import docking as D
    from pesto_amd.patches import _default_model
    K, U = int(c["off"][-1]), int(c["roff"][-1])
    F, Na, Nb = c["xa"].shape[0], c["xa"].shape[1], c["xb"].shape[1]
    model, lib = _default_model(0), _lib.load()
    xa, xb = place(on_device, c["xa"], c["xb"])
    side = _lib.Side(xa, model._gpu)
    if K >= 2:
        cap = K - 1
        off, pairs, d, sz = side.empty((F + 1,), np.int64), side.empty((cap + 8, 2), np.int32), side.empty((cap + 8,), np.float32), np.zeros(1, np.int64)
        pairs[cap:], d[cap:] = -7, -7.0
        _lib.check(lib.pesto_frame_contacts(model.handle, F, Na, Nb, side.ptr(xa), side.ptr(xb), c["r_thr"], c["scale"], cap, side.ptr(off),
                                            side.ptr(pairs), side.ptr(d), sz.ctypes.data, side.kind, side.stream), lib.pesto_docking_last_error)
        assert int(sz[0]) == K, (case, int(sz[0]), K)
        exact(case, "offsets at capacity K - 1", off, c["off"])
        assert np.all(host(pairs)[cap:] == -7) and np.all(host(d)[cap:] == -7.0), case
        got = D.frame_contacts(xa, xb, c["r_thr"], c["scale"], capacity=cap)
        for name, g, w in zip(("offsets", "pairs", "d"), got, (c["off"], c["pairs"], c["d"])):
            exact(case, f"{name} after the repeat", g, w)
    if U >= 2:
        cap = U - 1
        od, pd, dd = side.put(c["off"], np.int64), side.put(c["pairs"], np.int32), side.put(c["d"], np.float32)
        ra, rb = side.put(c["res_a"], np.int32), side.put(c["res_b"], np.int32)
        roff, rp, dm, sz = side.empty((F + 1,), np.int64), side.empty((cap + 8, 2), np.int32), side.empty((cap + 8,), np.float32), np.zeros(1, np.int64)
        rp[cap:], dm[cap:] = -7, -7.0
        _lib.check(lib.pesto_frame_residue_contacts(model.handle, F, Na, Nb, K, side.ptr(od), side.ptr(pd), side.ptr(dd), side.ptr(ra), side.ptr(rb),
                                                    int(c["res_a"].max()) + 1, int(c["res_b"].max()) + 1, cap, side.ptr(roff), side.ptr(rp), side.ptr(dm),
                                                    sz.ctypes.data, side.kind, side.stream), lib.pesto_docking_last_error)
        assert int(sz[0]) == U, (case, int(sz[0]), U)
        exact(case, "residue offsets at capacity U - 1", roff, c["roff"])
        assert np.all(host(rp)[cap:] == -7) and np.all(host(dm)[cap:] == -7.0), case


@pytest.mark.parametrize("case", S.DOCKING, ids=S.case_id)
def test_frame_contacts_residue_contacts_and_interface(case):
    from pesto_amd import docking as D
    c = S.build("docking", case)
    runs = []
    for on_device in sides("docking", case):
        xa, xb, xyz = place(on_device, c["xa"], c["xb"], c["xyz"])
        out = {}
        lists = D.frame_contacts(xa, xb, c["r_thr"], c["scale"])
        out["off"], out["pairs"], out["d"] = (host(v) for v in lists)
        out["roff"], out["rpairs"], out["dmin"] = (host(v) for v in D.frame_residue_contacts(xa, xb, c["res_a"], c["res_b"], c["r_thr"], c["scale"]))
        fed = D.frame_residue_contacts(lists, res_a=c["res_a"], res_b=c["res_b"])
        out["ira"], out["irb"] = (host(v) for v in D.interface_atoms(xyz, c["ids_a"], c["ids_b"], c["roa"], c["r_thr"], c["scale"]))
        for k in out:
            exact(case, k, out[k], c[k])
        for name, g, w in zip(("roff", "rpairs", "dmin"), fed, (c["roff"], c["rpairs"], c["dmin"])):
            exact(case, f"{name} from the lists", g, w)
        frames = D.contacts(xa, xb, c["ids_a"], c["ids_b"], c["r_thr"], c["scale"])
        assert len(frames) == c["off"].size - 1
        f = int(np.argmax(np.diff(c["off"])))
        lo, hi = c["off"][f], c["off"][f + 1]
        exact(case, f"contacts: d of frame {f}", frames[f][0], c["d"][lo:hi])
        exact(case, f"contacts: ids of frame {f}", frames[f][1], np.stack([c["ids_a"][c["pairs"][lo:hi, 0]], c["ids_b"][c["pairs"][lo:hi, 1]]], 1).astype(np.int32))
        contact_lists_with_a_small_capacity(case, c, on_device)
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


# ================================================================== pesto_amd.sasa
@pytest.mark.parametrize("case", S.SASA, ids=S.case_id)
def test_shrake_rupley(case):
    from pesto_amd import sasa as SA
    c = S.build("sasa", case)
    runs = []
    for on_device in sides("sasa", case):
        x, r = place(on_device, c["X"], c["R"])
        kw = dict(radii=r, probe_radius=0.0, n_sphere_points=c["P"], sizes=c["sizes"])
        area, counts = SA.shrake_rupley(x, return_counts=True, **kw)
        sums = SA.shrake_rupley(x, mode="residue", residue=c["rows"], **kw)
        out = dict(counts=host(counts), areas=host(area), sums=host(sums))
        for k in out:
            exact(case, k, out[k], c[k])
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


# ================================================================== pesto_cellgrid.h through both of its users
@pytest.fixture(scope="module")
def model():
    import torch
    from conftest import weights
    from pesto_amd import Model
    from pesto_amd.config import CONFIGS
    assert torch.cuda.is_available()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    return m


@pytest.mark.parametrize("case", S.CELLGRID, ids=S.case_id)
def test_cell_grid_contacts_and_labels(case, model):
    c = S.build("cellgrid", case)
    runs = []
    for on_device in sides("cellgrid", case):
        pairs, d, cties, labels, lties = run_cellgrid(model, c["asm"], on_device)
        out = dict(pairs=pairs, d=d, cties=cties, labels=labels, lties=lties)
        # against test_cellgrid's float64 brute force, the pairs within 1e-3 of r_thr left out
        key = lambda p: p[:, 0].astype(np.int64) * (1 << 32) + p[:, 1]      # noqa: E731
        got_far = pairs[~np.isin(key(pairs), key(c["band_pairs"]))].astype(np.int64)
        exact(case, "pairs outside the band against the float64 brute force", got_far, c["pairs64"][~c["near64"]])
        # against the float32 chain of dist(): the same pairs, d bit for bit, a tie flag exactly where d == r_thr
        exact(case, "pairs", pairs.astype(np.int64), c["pairs"])
        exact(case, "d", d, c["d"])
        exact(case, "contact ties", cties, c["ties"])
        exact(case, "label ties", lties, c["ties"])
        exact(case, "labelled residues", labels != 0, c["labelled"])
        assert set(np.unique(labels)) <= {0, 1}
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)


# ================================================================== kabsch_rotation through trajectory, irmsd and the rigid docking
@pytest.mark.parametrize("case", S.SUPERPOSE, ids=S.case_id)
def test_superposition_families(case):
    from pesto_amd import docking as D
    from pesto_amd import trajectory as T
    c = S.build("superpose", case)
    sel, ok = c["sel"], c["determined"]
    biggest = float(np.abs(c["xyz"]).max())
    runs = []
    for on_device in sides("superpose", case):
        y, x, yr, xr = place(on_device, c["ref"], c["xyz"], np.ascontiguousarray(c["ref"][:, sel]), np.ascontiguousarray(c["xyz"][:, sel]))
        t, R, tr = (host(v) for v in T.superpose_transform(yr, xr))
        sup, rm = host(T.superpose(y, x, sel, sel)), host(T.rmsd(y, x, sel, sel, scale=1.0))
        irm = host(D.irmsd(y, x, np.arange(c["half"]), np.arange(c["half"], c["roa"].size), c["roa"], c["ca"], r_thr=1e6, scale=1.0))
        dt, dr = (host(v) for v in D.interface_rigid_docking(y, x, sel, c["rest"], c["roa"], r_thr=1e6, scale=1.0))
        out = dict(t=t, R=R, tr=tr, sup=sup, rmsd=rm, irmsd=irm, dock_t=dt, dock_r=dr)
        # every frame: a finite proper rotation, and the selection's rmsd is the optimum
        assert all(np.isfinite(v).all() for v in out.values()), (case, [k for k, v in out.items() if not np.isfinite(v).all()])
        R64 = R.astype(np.float64)
        orth, det = np.abs(R64 @ np.swapaxes(R64, 1, 2) - np.eye(3)).max((1, 2)), np.abs(np.linalg.det(R64) - 1.0)
        print(f"{S.case_id(case)}: |R^T R - I| {orth.max():.2e}, |det R - 1| {det.max():.2e}, determined {ok.astype(int).tolist()}")
        assert (orth < 1e-6).all() and (det < 1e-6).all(), (case, orth, det)
        rm_bound = 4 * EPS32 * max(float(np.abs(c["rmsd64"]).max()), biggest)
        close(case, "rmsd", rm, c["rmsd64"], rm_bound)
        close(case, "irmsd", irm, c["irmsd64"], rm_bound)
        # one fit behind both: the same bits wherever the selection is not its reference's value for value (frames 1: of every family
        # but identity, whose frames all are), and there irmsd's identity short cut gives exactly 0
        moved = (c["xyz"][:, sel] != c["ref"][:, sel]).any((1, 2))
        assert moved[1:].all() or case[0] == "identity", case
        exact(case, "rmsd against irmsd off the reference", rm[moved], irm[moved])
        exact(case, "irmsd of a frame that is its reference", irm[~moved], np.zeros(int((~moved).sum()), np.float32))
        close(case, "t", t, c["t64"], bound4(c["t64"]))
        close(case, "t_ref", tr, c["tr64"], bound4(c["tr64"]))
        # where the covariance fixes the rotation: R, the superposed coordinates of all atoms, the rigid docking
        if ok.any():
            close(case, "R", R[ok], c["R64"][ok], bound4(c["R64"][ok]))
            close(case, "superposed xyz", sup[ok], c["sup64"][ok], bound4(c["sup64"][ok]))
            close(case, "rigid docking t", dt[ok], c["dock_t"][ok], bound4(c["dock_t"][ok]))
            close(case, "rigid docking r", dr[ok], c["dock_r"][ok], bound4(c["dock_r"][ok]))
        runs.append(out)
    if len(runs) == 2:
        same_bytes(case, *runs)
