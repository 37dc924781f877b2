"""GPU tests of pesto_amd.peaks (pesto_peaks.hip) against the NumPy definitions of test_peaks_fixture.py, through host arrays and ROCm
tensors. The interface centres within their derived bounds, the weight sums exact; distance_quantile bit for bit equal to a partition of
pdist32 over the seeded sweep (the 64-row block and the 256-column tile of the all-pairs skeleton from both sides), for points and for
the matrix, with contiguous, strided and permuted selections; density_peaks under the cut-off kernel equal to peaks_def in every output
(hand-worked cases, the sweep, a regular grid of exact ties, all three centre rules); under the Gaussian kernel rho within its bound,
everything after the density equal to the definition evaluated from the library's own rho, and equal to the float64 definition in every
decisive case; the matrix form, a second call and the other side give the same bits; bad inputs are refused; and the notebook's pipeline
on one ROCm tensor."""
import numpy as np
import pytest

from conftest import md_frames, weights
from test_peaks_fixture import (HAND_WORKED, SWEEP, centers_def, centers_tolerance, dc_of, grid_points, pdist32, peaks_def, quantile_rank, sweep_case,
                                sweep_points)

pytestmark = pytest.mark.gpu

ON = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def place(on_device, a):
    return dev(a) if on_device else a


def same_peaks(got, want, what, rho_exact=True):
    """every output of a Peaks result against a peaks_def dict: delta bit for bit, the rest exactly"""
    rho = host(got.rho)
    assert rho.dtype == np.float64 and host(got.delta).dtype == np.float32 and host(got.halo).dtype == np.bool_
    if rho_exact:
        assert np.array_equal(rho, want["rho"]), (what, "rho")
    assert np.array_equal(host(got.delta).view(np.uint32), want["delta"].view(np.uint32)), (what, "delta")
    for name, value in (("nh", got.nearest_higher), ("labels", got.labels), ("centers", got.centers), ("sizes", got.sizes)):
        v = host(value)
        assert v.dtype == np.int32 and np.array_equal(v, want[name]), (what, name, v, want[name])
    assert np.array_equal(host(got.halo), want["halo"]), (what, "halo")


def same_bits(a, b, what):
    assert a.dc == b.dc, what
    for x, y in zip(a[1:], b[1:]):
        x, y = host(x), host(y)
        assert x.dtype == y.dtype and x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)), what


def rules_of(n, dc):
    """the three centre rules as (arguments of density_peaks, arguments of peaks_def)"""
    K = min(3, n)
    return [(dict(n_clusters=K), dict(n_clusters=K)),
            (dict(rho_min=1.0, delta_min=2.0 * dc), dict(rho_min=1.0, delta_min=np.float32(2.0 * dc))),
            (dict(delta_factor=3.0), dict(rho_min=0.0, delta_min=np.float32(3.0 * dc)))]


# ---- interface centres
@pytest.mark.parametrize("R", [1, 63, 64, 65, 257, 1000])
@pytest.mark.parametrize("F", [1, 2, 65])
def test_interface_and_weighted_centers(F, R):
    from pesto_amd import peaks as K
    rng = np.random.default_rng(100 * F + R)
    Xp = (rng.normal(0.0, 3.0, (F, R, 3)) + rng.normal(0.0, 20.0, (F, 1, 3))).astype(np.float32)
    P = rng.uniform(0.0, 1.0, (F, R)).astype(np.float32)
    P[0, 0] = 0.9
    if R > 1:
        P[0, R // 2] = np.nan                   # compares false
    if F > 1:
        P[1] = np.minimum(P[1], 0.5)            # nothing above the threshold: 0.5 itself is not
    if F > 2:
        P[7] = 0.25
        P[7, R - 1] = 0.75                      # one residue: rg = 0
    with np.errstate(invalid="ignore"):
        T = (P > np.float32(0.5)).astype(np.float32)
    want_c, want_S, want_rg = centers_def(Xp, T)
    tol_c, tol_rg = centers_tolerance(Xp, T, want_c, want_rg)
    none = want_S == 0
    assert not none[0] and (F < 2 or none[1]) and (F < 3 or want_rg[7] == 0.0)
    results = []
    for on_device in (False, True):
        c, S, rg = K.interface_centers(place(on_device, Xp), place(on_device, P), 0.5)
        assert all(v.is_cuda if on_device else isinstance(v, np.ndarray) for v in (c, S, rg))
        c, S, rg = host(c), host(S), host(rg)
        assert c.dtype == np.float32 and S.dtype == np.float64 and rg.dtype == np.float32 and c.shape == (F, 3) and S.shape == rg.shape == (F,)
        assert np.array_equal(S, want_S)                                       # exact in threshold mode
        assert np.isnan(c[none]).all() and np.isnan(rg[none]).all() and not np.isnan(c[~none]).any() and not np.isnan(rg[~none]).any()
        err_c, err_rg = np.abs(c[~none] - want_c[~none]), np.abs(rg[~none] - want_rg[~none])
        print(f"F = {F}, R = {R}: centres {np.max(err_c / tol_c[~none]):.3f}, rg {np.max(err_rg / tol_rg[~none]):.3f} of their bounds")
        assert np.all(err_c <= tol_c[~none]) and np.all(err_rg <= tol_rg[~none])
        results.append((c, S, rg))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(*results))
    # the weights given directly: the soft weighting W = P
    W = np.nan_to_num(P, nan=0.0)
    if F > 1:
        W[1] = 0.0
    want_c, want_S, want_rg = centers_def(Xp, W)
    tol_c, tol_rg = centers_tolerance(Xp, W, want_c, want_rg)
    none = want_S == 0
    c, S, rg = (host(v) for v in K.weighted_centers(place(F % 2 == 0, Xp), place(F % 2 == 0, W)))
    assert np.all(np.abs(S - want_S) <= R * 2.0 ** -52 * want_S) and np.isnan(c[none]).all() and np.isnan(rg[none]).all()
    assert np.all(np.abs(c[~none] - want_c[~none]) <= tol_c[~none]) and np.all(np.abs(rg[~none] - want_rg[~none]) <= tol_rg[~none])
    again = [host(v) for v in K.weighted_centers(place(F % 2 == 0, Xp), place(F % 2 == 0, W))]
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip((c, S, rg), again))


@ON
def test_a_bad_weight_is_refused(on_device):
    from pesto_amd import peaks as K
    Xp = np.ones((3, 70, 3), np.float32)
    for bad in (-1.0, -1e-30, np.inf, np.nan):
        W = np.ones((3, 70), np.float32)
        W[2, 69] = bad
        with pytest.raises(ValueError, match="weight"):
            K.weighted_centers(place(on_device, Xp), place(on_device, W))
    c, S, rg = K.weighted_centers(place(on_device, Xp), place(on_device, np.ones((3, 70), np.float32)))
    assert host(S).tolist() == [70.0] * 3 and not host(rg).any() and np.array_equal(host(c), np.ones((3, 3), np.float32))


# ---- the pair distance of a given rank
@pytest.mark.parametrize("n,d", SWEEP)
def test_distance_quantile_equals_a_partition(n, d):
    from pesto_amd import peaks as K
    case = sweep_case(n, d)
    X, D = case["X"], case["D"]
    M = n * (n - 1) // 2
    for k_at, pdc in enumerate((1e-9, 2.0, 37.0, 100.0)):
        k = quantile_rank(n, pdc)
        assert (pdc != 1e-9 or k == 0) and (pdc != 100.0 or k == M - 1) and (n < 63 or pdc != 37.0 or 0 < k < M - 1)
        want = dc_of(D, k)
        on_device = (k_at + n + d) % 2 == 0
        got_x = K.distance_quantile(place(on_device, X), pdc=pdc)
        got_d = K.distance_quantile(D=place(not on_device, D), pdc=pdc)
        assert isinstance(got_x, float) and np.float32(got_x).view(np.uint32) == want.view(np.uint32), (n, d, pdc, got_x, want)
        assert np.float32(got_d).view(np.uint32) == want.view(np.uint32), (n, d, pdc, got_d, want)


def selection(kind, n, F, rng):
    if kind == "contiguous":
        return np.arange(3, 3 + n)
    if kind == "strided":
        return np.arange(1, 2 * n + 1, 2)
    return rng.permutation(F)[:n]


@ON
@pytest.mark.parametrize("kind", ["contiguous", "strided", "permuted"])
def test_selections(kind, on_device):
    from pesto_amd import peaks as K
    rng = np.random.default_rng(len(kind))
    F, n = 300, 129
    X = sweep_points(F, 3)
    D = pdist32(X)
    idx = selection(kind, n, F, rng)
    sub = pdist32(X[idx])
    assert np.array_equal(sub.view(np.uint32), D[np.ix_(idx, idx)].view(np.uint32))
    want_dc = dc_of(sub, quantile_rank(n, 5.0))
    for sel in (idx, place(on_device, idx.astype(np.int32))):
        assert K.distance_quantile(place(on_device, X), pdc=5.0, idx=sel) == float(want_dc)
        assert K.distance_quantile(D=place(on_device, D), pdc=5.0, idx=sel) == float(want_dc)
    mask = np.zeros(F, bool)
    mask[idx] = True
    assert K.distance_quantile(place(on_device, X), pdc=5.0, idx=mask) == float(dc_of(pdist32(X[mask]), quantile_rank(n, 5.0)))
    want = peaks_def(sub, want_dc, "cutoff", n_clusters=3)
    for got in (K.density_peaks(place(on_device, X), pdc=5.0, kernel="cutoff", n_clusters=3, idx=idx),
                K.density_peaks(D=place(on_device, D), pdc=5.0, kernel="cutoff", n_clusters=3, idx=idx)):
        assert got.dc == float(want_dc)
        same_peaks(got, want, kind)


@ON
def test_duplicated_points(on_device):
    from pesto_amd import peaks as K
    X = np.repeat(sweep_points(20, 3), 4, axis=0)           # 80 points, 120 pairs at distance 0 among 3160
    D = pdist32(X)
    assert K.distance_quantile(place(on_device, X), pdc=2.0) == 0.0 and K.distance_quantile(D=place(on_device, D), pdc=2.0) == 0.0
    pdc = 100.0 * 121 / 3160
    assert quantile_rank(80, pdc) == 120
    assert K.distance_quantile(place(on_device, X), pdc=pdc) == float(dc_of(D, 120)) > 0.0
    with pytest.raises(ValueError, match="is 0"):
        K.density_peaks(place(on_device, X), pdc=2.0, n_clusters=2)
    dc = float(dc_of(D, 400))
    for kernel in ("cutoff", "gaussian"):                   # exact ties in rho among the copies, resolved by index
        got = K.density_peaks(place(on_device, X), dc=dc, kernel=kernel, n_clusters=3)
        same_peaks(got, peaks_def(D, dc, kernel, n_clusters=3, rho=host(got.rho)), kernel)
        if kernel == "cutoff":
            same_peaks(got, peaks_def(D, dc, kernel, n_clusters=3), kernel)


# ---- density peaks, the cut-off kernel
@pytest.mark.parametrize("name", sorted(HAND_WORKED))
def test_hand_worked_cases(name):
    from pesto_amd import peaks as K
    case = HAND_WORKED[name]
    X, dc = case["X"], case["dc"]
    D = pdist32(X)
    for at, (rule, centers, labels, sizes, halo) in enumerate(case["rules"]):
        want = peaks_def(D, dc, "cutoff", **rule)
        for on_device in (False, True):
            for got in (K.density_peaks(place(on_device, X), dc=dc, kernel="cutoff", **rule),
                        K.density_peaks(D=place(on_device, D), dc=dc, kernel="cutoff", **rule)):
                assert all(v.is_cuda if on_device else isinstance(v, np.ndarray) for v in got[1:])
                same_peaks(got, want, (name, at))
                assert host(got.rho).tolist() == case["rho"] and host(got.nearest_higher).tolist() == case["nh"]
                assert host(got.centers).tolist() == centers and host(got.sizes).tolist() == sizes and np.nonzero(host(got.halo))[0].tolist() == halo
                assert labels is None or host(got.labels).tolist() == labels
                assert case["delta"] is None or host(got.delta).tolist() == case["delta"]


@pytest.mark.parametrize("n,d", SWEEP)
def test_cutoff_kernel_equals_the_definition(n, d):
    from pesto_amd import peaks as K
    case = sweep_case(n, d)
    X, D = case["X"], case["D"]
    pdc = 10.0
    dc = float(dc_of(D, quantile_rank(n, pdc)))
    for at, (rule, rule_def) in enumerate(rules_of(n, dc)):
        want = peaks_def(D, dc, "cutoff", **rule_def)
        on_device = (at + n + d) % 2 == 0
        got_x = K.density_peaks(place(on_device, X), pdc=pdc, kernel="cutoff", **rule)
        got_d = K.density_peaks(D=place(not on_device, D), dc=dc, kernel="cutoff", **rule)
        assert got_x.dc == dc and got_d.dc == dc
        same_peaks(got_x, want, (n, d, at, "points"))
        same_peaks(got_d, want, (n, d, at, "matrix"))
        assert int(host(got_x.sizes).sum()) == n and (at != 0 or len(host(got_x.centers)) == min(3, n))


def test_one_point_and_exact_ties():
    from pesto_amd import peaks as K
    one = K.density_peaks(np.array([[1.0, 2.0]], np.float32), dc=1.0, kernel="cutoff", n_clusters=1)
    assert host(one.rho).tolist() == [0.0] and host(one.delta).tolist() == [0.0] and host(one.nearest_higher).tolist() == [-1]
    assert host(one.labels).tolist() == [0] and host(one.centers).tolist() == [0] and host(one.sizes).tolist() == [1] and not host(one.halo).any()
    one = K.density_peaks(D=dev(np.zeros((1, 1), np.float32)), dc=0.5, kernel="gaussian", delta_min=0.0)
    assert host(one.centers).tolist() == [0] and host(one.sizes).tolist() == [1]
    # a regular grid: ties in rho and in distance throughout, every one resolved by index
    X = grid_points(9)
    D = pdist32(X)
    for dc in (1.0, 1.5, 2.5):
        for rule, rule_def in rules_of(81, dc)[:2] + [(dict(delta_min=0.0), dict(delta_min=np.float32(0.0)))]:
            want = peaks_def(D, dc, "cutoff", **rule_def)
            same_peaks(K.density_peaks(dev(X), dc=dc, kernel="cutoff", **rule), want, (dc, rule, "points"))
            same_peaks(K.density_peaks(D=D, dc=dc, kernel="cutoff", **rule), want, (dc, rule, "matrix"))
    every = K.density_peaks(X, dc=1.5, kernel="cutoff", delta_min=0.0)           # every point a centre
    assert host(every.sizes).tolist() == [1] * 81 and host(every.centers)[0] == 10


# ---- density peaks, the Gaussian kernel
@pytest.mark.parametrize("n,d", SWEEP)
def test_gaussian_kernel(n, d):
    from pesto_amd import peaks as K
    case = sweep_case(n, d)
    X, D, dc = case["X"], case["D"], case["dc"]
    for at, (rule, rule_def) in enumerate(rules_of(n, dc)):
        on_device = (at + n + d) % 2 == 0
        got = K.density_peaks(place(on_device, X), pdc=2.0, kernel="gaussian", **rule)
        assert got.dc == dc
        rho = host(got.rho)
        err = np.abs(rho - case["rho64"])
        if at == 0:
            with np.errstate(invalid="ignore", divide="ignore"):
                print(f"n = {n}, d = {d}: rho at most {np.nanmax(np.where(case['tol'] > 0, err / case['tol'], 0.0)):.3f} of its bound, decisive {case['decisive']}")
        assert np.all(err <= case["tol"]), (n, d)
        same_peaks(got, peaks_def(D, dc, "gaussian", rho=rho, **rule_def), (n, d, at, "own rho"))
        if case["decisive"]:
            same_peaks(got, peaks_def(D, dc, "gaussian", **rule_def), (n, d, at, "float64"), rho_exact=False)
        if d >= 2 and n >= 3:
            assert case["decisive"]
        # the matrix form gives the bits of the points form
        same_bits(K.density_peaks(D=place(not on_device, D), dc=dc, kernel="gaussian", **rule), got, (n, d, at))


# ---- consistency
@pytest.mark.parametrize("kernel", ["cutoff", "gaussian"])
def test_same_bits_again_and_on_the_other_side(kernel):
    from pesto_amd import peaks as K
    case = sweep_case(513, 3)
    X, D = case["X"], case["D"]
    first = K.density_peaks(X, pdc=2.0, kernel=kernel, n_clusters=3)
    for other in (K.density_peaks(X, pdc=2.0, kernel=kernel, n_clusters=3), K.density_peaks(dev(X), pdc=2.0, kernel=kernel, n_clusters=3),
                  K.density_peaks(dev(X), pdc=2.0, kernel=kernel, n_clusters=3), K.density_peaks(D=D, pdc=2.0, kernel=kernel, n_clusters=3),
                  K.density_peaks(D=dev(D), pdc=2.0, kernel=kernel, n_clusters=3)):
        same_bits(other, first, kernel)
    import torch
    t = torch.from_numpy(X)
    out = K.density_peaks(t, pdc=2.0, kernel=kernel, n_clusters=3)               # a CPU tensor in, CPU tensors out
    assert all(isinstance(v, torch.Tensor) and not v.is_cuda for v in out[1:])
    same_bits(out, first, kernel)


# ---- refusals
@ON
def test_bad_inputs_are_refused(on_device):
    from pesto_amd import _lib
    from pesto_amd import peaks as K
    X = sweep_points(70, 3)
    D = pdist32(X)
    refused = (ValueError, _lib.PestoError)
    for i, j, v in ((0, 1, 0.75), (69, 3, 0.75), (64, 65, None)):
        A = D.copy()
        A[i, j] = np.nextafter(A[i, j], np.float32(0)) if v is None else v
        with pytest.raises(refused, match="symmetric"):
            K.distance_quantile(D=place(on_device, A))
        with pytest.raises(refused, match="symmetric"):
            K.density_peaks(D=place(on_device, A), dc=1.0, n_clusters=2)
    for v, word in ((-1.0, "negative"), (np.nan, "finite"), (np.inf, "finite")):
        A = D.copy()
        A[5, 66] = A[66, 5] = v
        with pytest.raises(refused, match=word):
            K.distance_quantile(D=place(on_device, A))
        with pytest.raises(refused, match=word):
            K.density_peaks(D=place(on_device, A), dc=1.0, n_clusters=2)
        B = X.copy()
        B[69, 2] = v if v != -1.0 else np.nan
        with pytest.raises(refused, match="finite"):
            K.distance_quantile(place(on_device, B))
        with pytest.raises(refused, match="finite"):
            K.density_peaks(place(on_device, B), dc=1.0, n_clusters=2)
    A = D.copy()
    np.fill_diagonal(A, np.nan)                                                 # the diagonal is ignored
    assert K.distance_quantile(D=place(on_device, A)) == K.distance_quantile(place(on_device, X))
    with pytest.raises(refused):
        K.density_peaks(place(on_device, np.zeros((4, 9), np.float32)), dc=1.0, n_clusters=2)
    for dc in (0.0, -1.0):
        with pytest.raises(refused, match="dc"):
            K.density_peaks(place(on_device, X), dc=dc, n_clusters=2)
    for rule in (dict(), dict(n_clusters=2, delta_min=1.0)):
        with pytest.raises(refused, match="exactly one"):
            K.density_peaks(place(on_device, X), dc=1.0, **rule)
    with pytest.raises(refused, match="n_clusters"):
        K.density_peaks(place(on_device, X), dc=1.0, n_clusters=71)
    for idx in ([0, 70], [-1, 3]):
        with pytest.raises(refused, match="idx"):
            K.density_peaks(place(on_device, X), dc=1.0, n_clusters=2, idx=idx)
        with pytest.raises(refused, match="idx"):
            K.distance_quantile(D=place(on_device, D), idx=idx)


def test_the_library_checks_what_python_checks():
    """the C entry points refuse the same arguments themselves, and write nothing"""
    import ctypes
    from pesto_amd import _lib
    from pesto_amd.trajectory import _default_model
    lib, h = _lib.load(), _default_model(0).handle
    X = sweep_points(70, 3)
    idx = np.array([0, 70], np.int32)
    out = ctypes.c_float(-7.0)
    ptr = lambda a: a.ctypes.data
    assert lib.pesto_pair_distance_rank(h, 70, 3, ptr(X), None, 2, ptr(idx), 0, ctypes.byref(out), _lib.PTR_HOST, None) == -1
    assert b"idx" in lib.pesto_peaks_last_error() and out.value == -7.0
    assert lib.pesto_pair_distance_rank(h, 70, 9, ptr(X), None, 70, None, 0, ctypes.byref(out), _lib.PTR_HOST, None) == -1
    assert lib.pesto_pair_distance_rank(h, 70, 3, ptr(X), None, 70, None, 70 * 69 // 2, ctypes.byref(out), _lib.PTR_HOST, None) == -1
    assert lib.pesto_pair_distance_rank(h, 70, 3, ptr(X), ptr(X), 70, None, 0, ctypes.byref(out), _lib.PTR_HOST, None) == -1
    rho, delta = np.full(70, -7.0), np.full(70, -7.0, np.float32)
    ints = [np.full(70, -7, np.int32) for _ in range(4)]
    halo, nc = np.full(70, 7, np.uint8), ctypes.c_int32(-7)
    bad = X.copy()
    bad[3, 1] = np.inf
    for pts, dc, K_ in ((bad, 1.0, 2), (X, 0.0, 2), (X, 1.0, 71), (X, 1.0, 1025)):
        rc = lib.pesto_density_peaks(h, 70, 3, ptr(pts), None, 70, None, dc, 0, K_, 0.0, 0.0, ptr(rho), ptr(delta), ptr(ints[0]), ptr(ints[1]), ptr(halo),
                                     ptr(ints[2]), ptr(ints[3]), ctypes.byref(nc), _lib.PTR_HOST, None)
        assert rc == -1 and nc.value == -7 and (rho == -7.0).all() and (delta == -7.0).all() and all((v == -7).all() for v in ints) and (halo == 7).all()
    W = np.ones((2, 5), np.float32)
    W[1, 4] = -1.0
    c, S, rg, ones = np.full((2, 3), -7.0, np.float32), np.full(2, -7.0), np.full(2, -7.0, np.float32), np.ones((2, 5, 3), np.float32)
    assert lib.pesto_weighted_centers(h, 2, 5, ptr(ones), ptr(W), 1, 0.0, ptr(c), ptr(S), ptr(rg), _lib.PTR_HOST, None) == -1
    assert b"weight" in lib.pesto_peaks_last_error() and (c == -7.0).all() and (S == -7.0).all() and (rg == -7.0).all()


# ---- the notebook's pipeline on one ROCm tensor
def test_forward_frames_to_interface_clusters_on_the_device():
    from pesto_amd import Model
    from pesto_amd import peaks as K
    from pesto_amd import trajectory as T
    from pesto_amd.config import CONFIGS
    import torch
    f = md_frames("1JTG_uL")
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    roa = dev(f["res_of_atom"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), roa.long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    P = torch.sigmoid(z[:, :, 0]).contiguous()
    Xr = T.residue_centroids(X, f["res_of_atom"], f["R"], model=m)
    Xp = T.superpose(Xr[:1], Xr, model=m)
    assert P.is_cuda and Xp.is_cuda and tuple(Xp.shape) == (29, f["R"], 3)
    Ph, Xh = host(P), host(Xp)
    dropped = {}
    for p_thr in (0.15, 0.5):                   # every frame has a residue above 0.15; at 0.5 about half of them have none
        with np.errstate(invalid="ignore"):
            Th = (Ph > np.float32(p_thr)).astype(np.float32)
        want_c, want_S, want_rg = centers_def(Xh, Th)
        tol_c, tol_rg = centers_tolerance(Xh, Th, want_c, want_rg)
        keep = np.nonzero(want_S > 0)[0]
        dropped[p_thr] = 29 - keep.size
        for kernel in ("cutoff", "gaussian"):
            out = K.cluster_interface_frames(Xp, P, p_thr=p_thr, kernel=kernel, pdc=10.0, n_clusters=3, model=m)
            assert all(v.is_cuda for v in out[1:])
            Xc = host(out.Xc)
            assert np.array_equal(host(out.wsum), want_S)
            assert np.all(np.abs(Xc[keep] - want_c[keep]) <= tol_c[keep]) and np.all(np.abs(host(out.rg)[keep] - want_rg[keep]) <= tol_rg[keep])
            D = pdist32(Xc[keep])
            assert out.dc == float(dc_of(D, quantile_rank(keep.size, 10.0)))
            rho = host(out.rho)
            want = peaks_def(D, out.dc, kernel, n_clusters=3, rho=rho[keep] if kernel == "gaussian" else None)
            lost = np.setdiff1d(np.arange(29), keep)
            assert np.isnan(Xc[lost]).all() and np.isnan(rho[lost]).all() and np.isnan(host(out.delta)[lost]).all()
            assert (host(out.labels)[lost] == -1).all() and not host(out.halo)[lost].any() and (host(out.nearest_higher)[lost] == -1).all()
            assert np.array_equal(rho[keep], want["rho"])
            assert np.array_equal(host(out.delta)[keep].view(np.uint32), want["delta"].view(np.uint32))
            assert np.array_equal(host(out.labels)[keep], want["labels"]) and np.array_equal(host(out.halo)[keep], want["halo"])
            assert np.array_equal(host(out.centers), keep[want["centers"]]) and np.array_equal(host(out.sizes), want["sizes"])
            assert np.array_equal(host(out.nearest_higher)[keep], np.where(want["nh"] >= 0, keep[np.maximum(want["nh"], 0)], -1))
            assert host(out.centers).dtype == np.int32 and host(out.nearest_higher).dtype == np.int32
            picked = z[out.centers.long()]                                      # the centres' logits, never off the device
            assert picked.is_cuda and tuple(picked.shape) == (3, f["R"], z.shape[2])
    assert dropped[0.15] == 0 and 0 < dropped[0.5] < 29
    # host arrays in, host arrays out, the same result
    again = K.cluster_interface_frames(Xh, Ph, p_thr=0.5, kernel="gaussian", pdc=10.0, n_clusters=3)
    assert all(isinstance(v, np.ndarray) for v in again[1:]) and again.dc == out.dc
    for a, b in zip(again[1:], out[1:]):
        assert np.array_equal(a.view(np.uint8), host(b).view(np.uint8))
