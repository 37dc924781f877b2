"""GPU tests of pesto_amd.trajectory (pesto_trajectory.hip) against the reference's md_analysis/mdtraj_utils functions
(tests/golden/trajectory.npz): counts and P bit-equal through host arrays and ROCm tensors, for one and several frame splits and for
xyz1=None; a 1,235-atom self-distribution on the device; L, KL, the ensemble comparison, superposition, rmsd and centroids within
max(4 e_ref, 4 eps32 max|value|) of the float64 restatement, with identical bits from run to run; contact maps, native contacts and fnat
exactly; Model.forward_frames followed by centroids and superposition on the same ROCm tensor (the coordinates stay on the device; the
residue rows are ordered on the host); many frame splits, several log-likelihood passes, degenerate selections. For superposed coordinates
and centroids the float64 yardstick is test code (superpose64, centroids64 of test_trajectory_fixture.py), see there."""
import numpy as np
import pytest

from conftest import golden, md_frames, weights
from test_trajectory_fixture import (BINS, CONTACT_CASES, centroids64, contact_inputs, counts_def, from256, kl64, loglik64, p_of_counts,
                                     superpose64, superpose_inputs, tolerance)

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def place(on_device, *arrays):
    return [dev(a) if on_device else a for a in arrays]


def close(g, key, got, value64):
    got = host(got).astype(np.float64)
    assert got.shape == np.shape(value64), key
    tol = tolerance(g, key, value64)
    err = float(np.max(np.abs(got - value64)))
    print(f"{key}: max deviation {err:.3e}, bound {tol:.3e}")
    assert err <= tol, (key, err, tol)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("case", CONTACT_CASES)
def test_counts_and_distribution_bit_equal(case, on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    x0, x1, bins = contact_inputs(g, case)
    want = g[case + "_counts"].astype(np.uint32)
    want_p = p_of_counts(want)
    a, b = place(on_device, x0, x1)
    F = x0.shape[0]
    for splits in (None, 1, 2, 1000):                  # (at most 2 chunks of 32 frames here; more: test_many_frame_splits_add_up)
        c = T.contact_counts(a, b, bins=bins, frame_splits=splits)
        assert (c.is_cuda if on_device else isinstance(c, np.ndarray))
        assert np.array_equal(host(c).view(np.uint32), want), (case, splits)
        P = T.contacts_distribution(a, a if b is None else b, bins, frame_splits=splits)
        assert host(P).dtype == np.float32 and np.array_equal(host(P).view(np.uint32), want_p.view(np.uint32)), (case, splits)
    if x1 is None:                                      # xyz1=None is xyz0 against itself
        assert np.array_equal(host(T.contact_counts(a, a, bins=bins)).view(np.uint32), want)
    else:
        both = np.concatenate([x0, x1], 1)
        n = x0.shape[1]
        c = host(T.contact_counts(place(on_device, both)[0], bins=bins)).view(np.uint32)
        c2 = host(T.contact_counts(place(on_device, both)[0], place(on_device, both.copy())[0], bins=bins)).view(np.uint32)
        assert np.array_equal(c, c2) and np.array_equal(c[:n, n:], want) and np.array_equal(c[n:, :n], want.transpose(1, 0, 2))
    assert F == x0.shape[0]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_model_fit_and_loglikelihood(on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    xa, xb, bins = contact_inputs(g, "iface")
    ya, yb, _ = contact_inputs(g, "iface_other")
    P64 = p_of_counts(g["iface_counts"])

    class Traj:
        def __init__(self, xyz):
            self.xyz = xyz
    a, b, c, d = place(on_device, xa, xb, ya, yb)
    m = T.StatisticalContactsModel(0.0, 10.0, 21)
    assert np.array_equal(m.bins, BINS)
    m.fit(Traj(a), Traj(b))
    assert np.array_equal(host(m.P).view(np.uint32), P64.view(np.uint32))
    L0, L = m.loglikelihood(Traj(a), Traj(b)), m.loglikelihood(c, d)
    assert (L0.is_cuda if on_device else isinstance(L0, np.ndarray)) and host(L0).dtype == np.float32
    close(g, "iface_L0", L0, g["iface_L0_f64"])
    close(g, "iface_L", L, g["iface_L_f64"])
    assert np.array_equal(host(m.loglikelihood(a, b)), host(L0)) and np.array_equal(host(m.loglikelihood(c, d)), host(L))
    # a model of the trajectory against itself
    s = T.StatisticalContactsModel(0.0, 10.0, 21)
    s.fit(c)
    Ps = p_of_counts(counts_def(ya, None, bins))
    assert np.array_equal(host(s.P).view(np.uint32), Ps.view(np.uint32))
    Ls = host(s.loglikelihood(c)).astype(np.float64)
    want = loglik64(ya, ya, bins, Ps)
    assert np.abs(Ls - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_div_kl_and_ensemble_comparison(on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    xa, xb, _ = contact_inputs(g, "iface")
    ya, yb, _ = contact_inputs(g, "iface_other")
    P, Q = p_of_counts(g["iface_counts"]), p_of_counts(g["iface_other_counts"])
    p, q = place(on_device, P, Q)
    D = T.div_KL(q, p)
    close(g, "iface_KL", D, g["iface_KL_f64"])
    assert np.array_equal(host(T.div_KL(q, p)), host(D))
    assert np.abs(host(T.div_KL(p, p)).astype(np.float64) - kl64(P, P)).max() <= 4 * np.finfo(np.float32).eps * np.abs(kl64(P, P)).max()
    a, b, c, d = place(on_device, xa, xb, ya, yb)
    L0, Lrel, D2 = T.interface_ensemble_comparison(a, b, c, d)
    close(g, "iface_L0", L0, g["iface_L0_f64"])
    close(g, "iface_Lrel", Lrel, g["iface_Lrel_f64"])
    close(g, "iface_KL", D2, g["iface_KL_f64"])
    again = T.interface_ensemble_comparison(a, b, c, d, xmin=0.0, xmax=10.0, num_bins=21)
    for u, v in zip((L0, Lrel, D2), again):
        assert np.array_equal(host(u), host(v))


def test_large_self_distribution_on_the_device():
    import torch
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    x = from256(g["chain1_256"])
    F, N = x.shape[:2]
    assert N == 1235
    bins = np.linspace(0.0, 512.0, 65)                 # 64 bins that hold every distance of the fixture's +-128 A box
    xd = dev(x)
    c = T.contact_counts(xd, bins=bins)
    P = T.contacts_distribution(xd, xd, bins)
    assert c.is_cuda and P.is_cuda and tuple(c.shape) == (N, N, 64)
    assert torch.equal(c, c.transpose(0, 1)) and torch.equal(P, P.transpose(0, 1))
    assert bool((c.sum(-1) == F).all())
    idx = torch.arange(N, device=c.device)
    assert bool((c[idx, idx, 0] == F).all())           # every atom at distance 0 from itself
    rng = np.random.default_rng(5)
    i, j = rng.integers(0, N, 4096), rng.integers(0, N, 4096)
    d = np.sqrt(np.sum(np.square(x[:, i] - x[:, j]), -1)).astype(np.float64)        # [F, 4096]
    b = np.searchsorted(bins, d, side="right") - 1
    want = np.zeros((4096, 64), np.int64)
    for f in range(F):
        np.add.at(want, (np.arange(4096), b[f]), 1)
    ii, jj = dev(i), dev(j)
    assert np.array_equal(host(c[ii, jj]), want)
    assert np.array_equal(host(P[ii, jj]).view(np.uint32), p_of_counts(want).view(np.uint32))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_contact_maps_and_fnat_exact(on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    cases = [("iface10", from256(g["iface10_a256"], True), from256(g["iface10_b256"], True), g["iface10_res_a"], g["iface10_res_b"]),
             ("plantedmap", g["plantedmap_a"], g["plantedmap_b"], g["plantedmap_res_a"], g["plantedmap_res_b"])]
    for name, xa, xb, ra, rb in cases:
        a, b = place(on_device, xa, xb)
        for tag, r_thr in (("t5", 5.0), ("t41", 4.1)):
            want = g[f"{name}_{tag}_maps"]
            m = T.residue_contact_maps(a, b, ra, rb, r_thr=r_thr)
            assert (m.is_cuda if on_device else isinstance(m, np.ndarray))
            assert host(m).dtype == np.uint8 and np.array_equal(host(m), want), (name, tag)
            if name == "iface10":
                nat, fn = T.native_contacts(m[:1], m), T.fnat(m[:1], m)
                assert host(nat).dtype == np.int64 and np.array_equal(host(nat), g[f"iface10_{tag}_native"])
                assert host(fn).dtype == np.float64 and np.array_equal(host(fn), g[f"iface10_{tag}_fnat"])
                full = T.fnat(m, m)                     # a reference frame per frame: the denominator counts them all
                assert np.array_equal(host(full), want.sum((1, 2)) / want.sum())
    # residue rows in any order: the maps follow the rows
    name, xa, xb, ra, rb = cases[0]
    perm = np.random.default_rng(3).permutation(xa.shape[1])
    a, b = place(on_device, xa[:, perm], xb)
    assert np.array_equal(host(T.residue_contact_maps(a, b, ra[perm], rb)), g["iface10_t5_maps"])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("tag", ["all", "sel", "mirror"])
def test_superposition_and_rmsd(tag, on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    ref, xyz, sel = superpose_inputs(g, tag)
    y, x = place(on_device, ref, xyz)
    yr, xr = (ref, xyz) if sel is None else (ref[:, sel], xyz[:, sel])
    t64, R64, tr64 = superpose64(yr, xr)
    sup64 = (xyz.astype(np.float64) - t64) @ R64 + tr64
    t, R, tr = T.superpose_transform(*place(on_device, yr, xr))
    assert tuple(t.shape) == (xyz.shape[0], 1, 3) and tuple(R.shape) == (xyz.shape[0], 3, 3) and tuple(tr.shape) == (1, 1, 3)
    close(g, f"superpose_{tag}_t", t, t64)
    close(g, f"superpose_{tag}_R", R, R64)
    close(g, f"superpose_{tag}_tref", tr, tr64)
    sup = T.superpose(y, x, sel, sel)
    assert (sup.is_cuda if on_device else isinstance(sup, np.ndarray))
    close(g, f"superpose_{tag}_xyz", sup, sup64)
    rm = T.rmsd(y, x, sel, sel)
    close(g, f"superpose_{tag}_rmsd", rm, g[f"superpose_{tag}_rmsd_f64"])
    assert np.array_equal(host(T.superpose(y, x, sel, sel)), host(sup)) and np.array_equal(host(T.rmsd(y, x, sel, sel)), host(rm))
    if sel is not None:                                 # a mask selects the same atoms
        mask = np.zeros(xyz.shape[1], bool)
        mask[sel] = True
        assert np.array_equal(host(T.superpose(y, x, mask, mask)), host(sup))
    if tag == "all":                                    # a reference frame per frame
        yy = place(on_device, np.repeat(ref, xyz.shape[0], 0))[0]
        assert np.array_equal(host(T.superpose(yy, x)), host(sup))
        close(g, "superpose_all_rmsd", host(T.rmsd(y, x, scale=1.0)).astype(np.float64) * 10.0, g["superpose_all_rmsd_f64"])


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_residue_centroids(on_device):
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    f = md_frames()
    X, roa, R = f["X_frames"], f["res_of_atom"], f["R"]
    want = centroids64(X, roa)
    x, r = place(on_device, X, roa)
    c = T.residue_centroids(x, r, R)
    assert (c.is_cuda if on_device else isinstance(c, np.ndarray)) and tuple(c.shape) == (X.shape[0], R, 3)
    close(g, "centroids", c, want)
    assert np.array_equal(host(T.residue_centroids(x, roa, R)), host(c))
    extra = host(T.residue_centroids(x, r, R + 2))       # rows without atoms
    assert np.array_equal(extra[:, :R], host(c)) and np.isnan(extra[:, R:]).all()


def test_forward_frames_then_centroids_and_superposition_on_the_device():
    import torch
    from pesto_amd import Model
    from pesto_amd import trajectory as T
    from pesto_amd.config import CONFIGS
    f = md_frames()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    roa = dev(f["res_of_atom"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), roa.long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    Xp = T.residue_centroids(X, roa, f["R"], model=m)
    Xs = T.superpose(Xp[:1], Xp, model=m)
    assert z.is_cuda and Xp.is_cuda and Xs.is_cuda and tuple(Xs.shape) == (X.shape[0], f["R"], 3)
    assert np.abs(host(z) - f["z"]).max() < 1e-4
    # the same through separate host calls
    Xp_h = T.residue_centroids(f["X_frames"], f["res_of_atom"], f["R"])
    assert np.array_equal(host(Xp), Xp_h) and np.array_equal(host(Xs), T.superpose(Xp_h[:1], Xp_h))
    t64, R64, tr64 = superpose64(Xp_h[:1], Xp_h)
    want = (Xp_h.astype(np.float64) - t64) @ R64 + tr64
    assert np.abs(host(Xs) - want).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()


@pytest.mark.parametrize("case,repeat", [("iface", 4), ("planted_b64", 22), ("planted_self", 22)])
def test_many_frame_splits_add_up(case, repeat):
    """the frames repeated until they fill several 32-frame chunks: 3, 8 and as many splits as there are chunks, added with integer
    atomics, give `repeat` times the fixture's counts, as one split does"""
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    x0, x1, bins = contact_inputs(g, case)
    want = g[case + "_counts"].astype(np.uint32) * np.uint32(repeat)
    a = dev(np.tile(x0, (repeat, 1, 1)))
    b = None if x1 is None else dev(np.tile(x1, (repeat, 1, 1)))
    chunks = -(-x0.shape[0] * repeat // 32)
    assert chunks >= 3
    for splits in (1, 3, 8, 1000, None):
        c = host(T.contact_counts(a, b, bins=bins, frame_splits=splits)).view(np.uint32)
        assert np.array_equal(c, want), (case, splits)
    ah = np.tile(x0, (repeat, 1, 1))
    bh = None if x1 is None else np.tile(x1, (repeat, 1, 1))
    assert np.array_equal(T.contact_counts(ah, bh, bins=bins, frame_splits=chunks), want)       # staged from the host


def test_loglikelihood_in_several_passes():
    """1,521 tiles x 5,632 frames of partials exceed one pass of the log-likelihood's scratch: the frames go through in two passes, and
    since they are the fixture's 8 frames repeated, L repeats with period 8, bit for bit, and equals the float64 restatement"""
    from pesto_amd import trajectory as T
    g = golden("trajectory")
    x = from256(g["chain1_256"])
    F0, N = x.shape[:2]
    repeat = 704
    assert (-(-N // 32)) ** 2 * F0 * repeat * 8 > 64 << 20
    m = T.StatisticalContactsModel(0.0, 10.0, 21)
    xs = dev(x)
    m.fit(xs)
    L8 = host(m.loglikelihood(xs))
    L = host(m.loglikelihood(dev(np.tile(x, (repeat, 1, 1)))))
    assert L.shape == (F0 * repeat,) and np.array_equal(L, np.tile(L8, repeat))
    i = np.arange(0, N, 5)                              # the restatement on a sub-block of the atoms, with the same model rows
    sub = T.StatisticalContactsModel(0.0, 10.0, 21)
    sub.fit(x[:, i])
    want = loglik64(x[:, i], x[:, i], BINS, host(sub.P))
    got = sub.loglikelihood(np.tile(x[:, i], (3, 1, 1))).astype(np.float64)
    assert np.abs(got - np.tile(want, 3)).max() <= 4 * np.finfo(np.float32).eps * np.abs(want).max()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_degenerate_selection_gives_a_finite_proper_rotation(on_device):
    """collinear atoms (rank-1 covariance) and coincident atoms (rank 0) leave the rotation undetermined: like an SVD library the fit
    returns some proper rotation, never NaN; the selection's rmsd, which does not depend on the choice, equals the float64 one within
    4 eps32 of the largest value (the result is rounded to float32 once)"""
    from pesto_amd import trajectory as T
    rng = np.random.default_rng(9)
    line = (np.linspace(-2.0, 2.0, 7)[:, None] * np.array([0.6, -0.3, 0.74]))[None] + np.array([3.0, 1.0, -2.0])
    ref = np.concatenate([line, rng.normal(0, 1, (1, 5, 3))], 1).astype(np.float32)                 # 7 collinear atoms + 5 others
    xyz = np.stack([ref[0] @ np.linalg.qr(rng.normal(0, 1, (3, 3)))[0] + rng.normal(0, 0.01, (12, 3)) for _ in range(4)]).astype(np.float32)
    xyz[:, :7] = xyz[:, :1] + (xyz[:, 6:7] - xyz[:, :1]) * np.linspace(0.0, 1.0, 7)[None, :, None].astype(np.float32)
    xyz[3, :7] = xyz[3, :1]                                                                         # frame 3: the selection in one point
    sel = np.arange(7)
    y, x = place(on_device, ref, xyz)
    sup, rm = host(T.superpose(y, x, sel, sel)), host(T.rmsd(y, x, sel, sel, scale=1.0)).astype(np.float64)
    assert np.isfinite(sup).all() and np.isfinite(rm).all()
    t, R, tr = (host(v).astype(np.float64) for v in T.superpose_transform(*place(on_device, ref[:, sel], xyz[:, sel])))
    assert np.abs(R @ np.swapaxes(R, 1, 2) - np.eye(3)).max() < 1e-6 and np.abs(np.linalg.det(R) - 1.0).max() < 1e-6
    t64, R64, tr64 = superpose64(ref[:, sel], xyz[:, sel])
    gap = (xyz[:, sel].astype(np.float64) - t64) @ R64 + tr64 - ref[:, sel].astype(np.float64)
    want = np.sqrt((gap * gap).sum(-1).mean(-1))
    assert np.abs(rm - want).max() <= 4 * np.finfo(np.float32).eps * max(np.abs(want).max(), np.abs(xyz).max())
