"""GPU tests of pesto_amd.normalmodes (pesto_enm.hip) against the float64 yardstick of test_normalmodes_fixture.py. Bounds are formulas
that hold for any order of summation (eps = 2^-52, gamma_p = p eps / (1 - p eps)): the list by equality of offsets and j, k equal for
p = 0 and within 4 eps k for p = 2; a dense entry within 8 eps k_ij off the diagonal blocks and gamma_{deg_i + 8} sum_j k_ij on them, the
matrices bitwise symmetric; a result of anm / gnm through check_modes (orthonormality and the rigid motions within 4 x LAPACK's own
deviation, the reported residuals against those recomputed with H64 within the 2-norm of the Hessian's entrywise bound plus 4 e_ref,
converged, Weyl, the sign rule, n_zero, bound == b; e_ref and the deviations carry the floors that test_normalmodes_fixture.py states). A sweep runs n over the edges of the layouts (the 64-wide
tile, 3n - 6 at 63 and 66 around the block of 64 vectors, rows of 0, 1, 63, 64 and 65 neighbours), p 0 and 2, a selection and both
scales; then the named cases of tests/golden/normalmodes.npz, what is derived from modes, the composition with dynamics.pca, bitwise
repeatability on both sides, refusals and non-convergence."""
import ctypes

import numpy as np
import pytest

from conftest import golden
from test_normalmodes_fixture import EPS64, NAMES, Network, ca_1thf, chain, check_modes, gamma, named, ratio_to

pytestmark = pytest.mark.gpu

SWEEP_N = [1, 2, 3, 4, 21, 22, 23, 24, 64, 65, 130]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def hub(n_shell, n_outer, seed, cutoff):
    """a hub, n_shell nodes on a sphere of 0.95 cutoff about it (the hub's row holds them all), n_outer on a sphere of 1.8 cutoff"""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((n_shell + n_outer, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    u[:n_shell] *= 0.95 * cutoff
    u[n_shell:] *= 1.8 * cutoff
    return np.ascontiguousarray(np.vstack([np.zeros((1, 3)), u]).astype(np.float32))


def sweep_input(n):
    """(coordinates float32 [n, 3] in angstroms, cutoff): chains at 12 A up to 24 nodes (every pair of up to 4 nodes is a spring), then hubs
    whose rows hold 63, 64 and 65 neighbours"""
    if n <= 24:
        return chain(n, 500 + n), 12.0
    return {64: hub(63, 0, 564, 14.0), 65: hub(64, 0, 565, 14.0), 130: hub(65, 64, 630, 14.0)}[n], 14.0


_sweep = {}


def swept(n, kind, p):
    """(xyz as passed, sel, scale, cutoff, Network): odd n in nanometres at scale 10, n % 4 == 1 or 2 behind a selection"""
    if (n, kind, p) not in _sweep:
        x, cutoff = sweep_input(n)
        scale = 10.0 if n % 2 else 1.0
        x = np.ascontiguousarray((x / np.float32(scale)).astype(np.float32))
        sel, xyz = None, x
        if n % 4 in (1, 2):
            xyz = np.ascontiguousarray(np.vstack([x[:1] + np.float32(0.5), x[::-1], x[-1:] * np.float32(3)]))
            sel = np.arange(n, 0, -1)
            if n % 4 == 2:
                xyz, sel = np.ascontiguousarray(np.vstack([x[:2], x[:1] + np.float32(0.25), x[2:]])), np.arange(n + 1) != 2
        _sweep[n, kind, p] = (xyz, sel, scale, cutoff, Network(x, kind, cutoff, scale, 1.5, p))
    return _sweep[n, kind, p]


@pytest.mark.parametrize("n", SWEEP_N)
def test_sweep_network_and_matrices(n):
    from pesto_amd import normalmodes as nm
    rows = set()
    for p in (0, 2):
        xyz, sel, scale, cutoff, net = swept(n, "anm", p)
        off, j, k = nm.network(xyz, sel=sel, cutoff=cutoff, scale=scale, gamma=1.5, p=p)
        o64, j64, k64 = net.csr()
        assert off.dtype == np.int64 and j.dtype == np.int32 and k.dtype == np.float64
        assert np.array_equal(off, o64) and np.array_equal(j, j64), (n, p)
        if p == 0:
            assert np.array_equal(k, k64)
        r_k = ratio_to(np.abs(k - k64), 4.0 * EPS64 * k64)
        rows |= set(np.diff(off).tolist())
        H = nm.hessian(xyz, sel=sel, cutoff=cutoff, scale=scale, gamma=1.5, p=p)
        G = nm.kirchhoff(xyz, sel=sel, cutoff=cutoff, scale=scale, gamma=1.5, p=p)
        assert H.shape == (3 * n, 3 * n) and G.shape == (n, n) and H.dtype == np.float64 and G.dtype == np.float64
        assert np.array_equal(H.view(np.uint64), H.T.view(np.uint64)) and np.array_equal(G.view(np.uint64), G.T.view(np.uint64))
        gnet = swept(n, "gnm", p)[4]
        r_h, r_g = ratio_to(np.abs(H - net.M), net.entry_bound()), ratio_to(np.abs(G - gnet.M), gnet.entry_bound())
        print("n", n, "p", p, "ratios k, H, Gamma", r_k, r_h, r_g)
        assert r_k <= 1.0 and r_h <= 1.0 and r_g <= 1.0, (n, p, r_k, r_h, r_g)
    want = {1: {0}, 2: {1}, 64: {63}, 65: {64}, 130: {65}}.get(n, set())
    assert want <= rows, (n, sorted(rows))


@pytest.mark.parametrize("n", [v for v in SWEEP_N if v >= 2])
def test_sweep_modes(n):
    from pesto_amd import normalmodes as nm
    for kind, p in (("anm", 0), ("anm", 2), ("gnm", 0), ("gnm", 2)):
        if kind == "anm" and n < 3:
            continue
        xyz, sel, scale, cutoff, net = swept(n, kind, p)
        room = 3 * n - 6 if kind == "anm" else n - 1
        e_ref, devs = net.e_ref(), net.lapack_dev()
        lam = net.eig()[0]
        assert not np.any((lam > 1e-14 * net.b) & (lam < 1e-6 * net.b)), (n, kind, lam[:8] / net.b)
        for k in [v for v in (1, 6, 20, 32) if v <= room]:
            res = (nm.anm if kind == "anm" else nm.gnm)(xyz, n_modes=k, sel=sel, cutoff=cutoff, scale=scale, gamma=1.5, p=p)
            check_modes(res, net, k, 1e-10, e_ref, devs, n_zero=int((lam[:k] <= 1e-10 * net.b).sum()), label=f"{kind} n={n} p={p} k={k}")


@pytest.mark.parametrize("case", NAMES)
def test_named_cases(case):
    from pesto_amd import normalmodes as nm
    (x, kind, cutoff, scale, p, k, nz), net, rec = named(case)
    res = (nm.anm if kind == "anm" else nm.gnm)(dev(x), n_modes=k, cutoff=cutoff, scale=scale, p=p)
    res = res._replace(eigenvalues=host(res.eigenvalues), modes=host(res.modes), residuals=host(res.residuals))
    check_modes(res, net, k, 1e-10, float(rec["e_ref"]), tuple(rec["dev"]), n_zero=nz, label=case)
    assert np.abs(res.eigenvalues - rec["lam"]).max() <= res.residuals.max() + 8.0 * float(rec["e_ref"])


_thf = {}


def thf_modes():
    if not _thf:
        from pesto_amd import normalmodes as nm
        _thf["x"] = ca_1thf()
        _thf["res"] = nm.anm(_thf["x"], n_modes=20, cutoff=15.0, scale=1.0)
    return _thf["x"], _thf["res"]


def test_derived_fluctuations_correlation_overlap():
    from pesto_amd import normalmodes as nm
    x, res = thf_modes()
    k, n = 20, len(x)
    lam, V = res.eigenvalues, res.modes
    fl = nm.mode_fluctuations(lam, V, factor=2.5)
    terms = (V * V).sum(2) / lam[:, None]
    want = 2.5 * terms.sum(0)
    r_f = ratio_to(np.abs(fl - want), gamma(3 * k + 2) * 2.5 * np.abs(terms).sum(0))
    assert fl.dtype == np.float64 and fl.shape == (n,) and r_f <= 1.0, r_f
    C = nm.mode_correlation(dev(lam), dev(V))
    C = host(C)
    cov = np.einsum("kia,kja->ij", V / lam[:, None, None], V)
    d = np.sqrt(np.diag(cov))
    assert C.dtype == np.float32 and np.array_equal(C.view(np.uint32), C.T.view(np.uint32)) and np.all(np.diag(C) == 1.0)
    r_c = float(np.abs(C.astype(np.float64) - cov / np.outer(d, d)).max() / 2.0 ** -23)
    assert r_c <= 1.0, r_c
    # a node without fluctuation gets 0, never NaN; a zero eigenvalue is left out of both sums
    V0 = V.copy()
    V0[:, 5] = 0.0
    lam0 = lam.copy()
    lam0[0] = 0.0
    C0, f0 = nm.mode_correlation(lam0, V0), nm.mode_fluctuations(lam0, V0)
    assert np.all(np.isfinite(C0)) and not C0[5, :5].any() and not C0[6:, 5].any() and C0[5, 5] == 1.0 and f0[5] == 0.0
    assert ratio_to(np.abs(f0 - ((V0 * V0).sum(2)[1:] / lam[1:, None]).sum(0)), gamma(3 * k + 2) * f0) <= 1.0
    # overlaps: modes against modes, and against a displacement
    rng = np.random.default_rng(5)
    B = rng.standard_normal((7, n, 3))
    ov = nm.overlap(V, B)
    A2, B2 = V.reshape(k, -1), B.reshape(7, -1)
    r_o = ratio_to(np.abs(ov - np.abs(A2 @ B2.T)), gamma(3 * n) * (np.abs(A2) @ np.abs(B2).T))
    assert ov.shape == (k, 7) and r_o <= 1.0, r_o
    self_ov = nm.overlap(V, V)
    assert np.abs(self_ov - np.eye(k)).max() <= 64 * EPS64
    disp = 0.6 * V[0] - 0.8 * V[3]
    o1 = nm.overlap(V, 7.0 * disp)
    assert o1.shape == (k, 1) and abs(o1[0, 0] - 0.6) <= 1e-14 and abs(o1[3, 0] - 0.8) <= 1e-14
    assert abs(nm.cumulative_overlap(o1[:, 0])[-1] - 1.0) <= 1e-14
    gm = nm.gnm(x, n_modes=5, cutoff=10.0, scale=1.0)
    fg = nm.mode_fluctuations(gm.eigenvalues, gm.modes)
    tg = gm.modes * gm.modes / gm.eigenvalues[:, None]
    assert ratio_to(np.abs(fg - tg.sum(0)), gamma(3 * 5 + 2) * tg.sum(0)) <= 1.0
    print("ratios fluctuations, correlation (ulp32 of 1), overlap", r_f, r_c, r_o)


def test_deform_and_structure_modes():
    from pesto_amd import normalmodes as nm
    x, res = thf_modes()
    g = golden("io_1thf_D")
    d = dict(xyz=g["final_xyz"], name=g["final_name"].astype(str), resid=g["final_resid"], chain_name=g["final_chain_name"].astype(str),
             resname=g["final_resname"].astype(str))
    sm, xyz, node = nm.structure_modes(d, n_modes=6, cutoff=15.0)
    assert xyz.shape == (1949, 3) and node.shape == (1949,) and node.dtype == np.int32 and node.min() == 0 and node.max() == 252
    ca_rows = np.nonzero(np.char.strip(d["name"]) == "CA")[0]
    assert np.array_equal(node[ca_rows], np.arange(253)) and np.all(np.diff(node) >= 0)
    assert sm.converged and sm.modes.shape == (6, 253, 3)
    A = nm.sample_amplitudes(sm.eigenvalues, 5, rmsd=1.0, seed=3, n_nodes=253)
    for noa, base, V in ((None, x, res.modes[:6]), (node, xyz, sm.modes)):
        out = nm.deform(dev(base), dev(V), dev(A), None if noa is None else dev(noa))
        out = host(out)
        Vn = V if noa is None else V[:, noa]
        terms = A[:, :, None, None] * Vn[None]
        want = base.astype(np.float64)[None] + terms.sum(1)
        bound = gamma(6 + 1) * np.abs(terms).sum(1) + np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        r_d = ratio_to(np.abs(out.astype(np.float64) - want), bound)
        print("deform ratio", r_d)
        assert out.dtype == np.float32 and out.shape == (5,) + base.shape and r_d <= 1.0, r_d
        assert np.array_equal(out.view(np.uint32), nm.deform(base, V, A, noa).view(np.uint32))           # host and device inputs: the same bits


def test_composition_with_pca():
    from pesto_amd import dynamics as dy, normalmodes as nm
    x, res = thf_modes()
    A = nm.mode_path(20, 0, 9, rmsd=1.0, n_nodes=len(x))
    frames = nm.deform(dev(x), dev(res.modes), dev(A))
    pc = dy.pca(frames, n_components=1, scale=1.0)
    loss = 1.0 - abs(float((host(pc.components)[0] * res.modes[0]).sum()))
    print("1 - |v . c| =", loss)
    assert loss <= 1e-6, loss
    assert float(host(nm.overlap(dev(res.modes[:1]), pc.components))[0, 0]) >= 1.0 - 1e-6


def test_same_bits_twice_and_on_both_sides():
    from pesto_amd import normalmodes as nm
    x, res = thf_modes()

    def bits(r):
        return [host(a).view(np.uint64) for a in (r.eigenvalues, r.modes, r.residuals)] + [np.array([r.bound]).view(np.uint64),
                                                                                            np.array([r.n_zero, r.iterations, r.applies, r.n_springs])]
    for other in (nm.anm(x, n_modes=20, cutoff=15.0, scale=1.0), nm.anm(dev(x), n_modes=20, cutoff=15.0, scale=1.0)):
        assert all(np.array_equal(a, b) for a, b in zip(bits(res), bits(other)))
    g1, g2 = nm.gnm(x, n_modes=7, scale=1.0), nm.gnm(dev(x), n_modes=7, scale=1.0)
    assert all(np.array_equal(a, b) for a, b in zip(bits(g1), bits(g2)))
    for f in (nm.hessian, nm.kirchhoff):
        a, b = f(x[:70], scale=1.0, p=2), host(f(dev(x[:70]), scale=1.0, p=2))
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64)) and np.array_equal(a.view(np.uint64), f(x[:70], scale=1.0, p=2).view(np.uint64))
    n1, n2 = nm.network(x, scale=1.0, p=2), nm.network(dev(x), scale=1.0, p=2)
    assert all(np.array_equal(a, host(b)) for a, b in zip(n1, n2))


def test_cutoff_is_strict_on_the_device():
    from pesto_amd import normalmodes as nm
    at = np.array([[0, 0, 0], [8, 0, 0], [8, 0, 0]], np.float32)          # a pair at exactly the cut-off on dyadic coordinates; two coincident nodes
    near = at.copy()
    near[1:, 0] = np.nextafter(np.float32(8), np.float32(0))              # one float32 step nearer
    for x, scale in ((at, 1.0), (at / 8, 8.0)):
        assert nm.network(x, cutoff=8.0, scale=scale)[0].tolist() == [0, 0, 0, 0] and not nm.hessian(x, cutoff=8.0, scale=scale).any()
    off, j, k = nm.network(near, cutoff=8.0, scale=1.0)
    assert off.tolist() == [0, 2, 3, 4] and j.tolist() == [1, 2, 0, 0] and k.tolist() == [1.0] * 4


def test_refusals_leave_outputs_untouched():
    from pesto_amd import _lib, normalmodes as nm
    from pesto_amd.trajectory import _model_of
    x = chain(24, 524)
    bad = x.copy()
    bad[7, 1] = np.nan
    for f in (nm.anm, nm.gnm, nm.network, nm.hessian, nm.kirchhoff):
        with pytest.raises((ValueError, _lib.PestoError)):
            f(bad, cutoff=12.0, scale=1.0)
        with pytest.raises((ValueError, _lib.PestoError)):
            f(dev(bad), cutoff=12.0, scale=1.0)
    assert nm.network(bad, sel=np.arange(24) != 7, cutoff=12.0, scale=1.0)[0][-1] > 0          # outside the selection a NaN is nobody's business
    with pytest.raises(ValueError):
        nm.anm(x, n_modes=33, cutoff=12.0, scale=1.0)
    with pytest.raises(ValueError):
        nm.anm(x[:3], n_modes=4, cutoff=12.0, scale=1.0)
    # through the C entry point, prefilled outputs on the device: an index out of range, a NaN, n_modes out of range
    import torch
    lib, model = _lib.load(), _model_of(None, x)
    h, stream = model.handle, torch.cuda.current_stream().cuda_stream
    k = 5
    eig, modes, resid = (torch.full(s, 7.25, dtype=torch.float64, device="cuda:0") for s in ((k,), (k, 24, 3), (k,)))
    b, K, info = ctypes.c_double(-1.0), ctypes.c_int64(-1), (ctypes.c_int32 * 6)(*([-1] * 6))

    def modes_call(xd, seld, n_sel, kk):
        return lib.pesto_enm_modes(h, 24, n_sel, xd.data_ptr(), None if seld is None else seld.data_ptr(), 12.0, 1.0, 1.0, 0, 3, kk, 1e-10, 32,
                                   eig.data_ptr(), modes.data_ptr(), resid.data_ptr(), ctypes.byref(b), ctypes.byref(K), info, _lib.PTR_DEVICE, stream)
    xd, badd = dev(x), dev(bad)
    sel_bad = dev(np.array([0, 1, 2, 24, 4], np.int32))
    for rc in (modes_call(xd, sel_bad, 5, k), modes_call(badd, None, 24, k), modes_call(xd, None, 24, 33), modes_call(xd, None, 24, 0)):
        assert rc == -1 and lib.pesto_enm_last_error()
        torch.cuda.synchronize()
        assert all(bool((t == 7.25).all()) for t in (eig, modes, resid)) and b.value == -1.0 and K.value == -1 and info[0] == -1
    out = torch.full((3, 24, 3), 7.25, dtype=torch.float32, device="cuda:0")
    nodes = dev(np.array([0] * 23 + [24], np.int32))
    amp, md = dev(np.zeros((3, k))), dev(np.zeros((k, 24, 3)))
    rc = lib.pesto_enm_deform(h, 3, 24, 24, k, xd.data_ptr(), md.data_ptr(), amp.data_ptr(), nodes.data_ptr(), out.data_ptr(), _lib.PTR_DEVICE, stream)
    torch.cuda.synchronize()
    assert rc == -1 and bool((out == 7.25).all())
    # the handle serves the next call
    assert modes_call(xd, None, 24, k) == 0 and info[2] == 1 and bool(torch.isfinite(modes).all()) and b.value > 0


def test_non_convergence_is_reported():
    from pesto_amd import normalmodes as nm
    x, res = thf_modes()
    one = nm.anm(x, n_modes=20, cutoff=15.0, scale=1.0, max_iter=1)
    assert one.converged is False and one.iterations == 1 and one.applies == 1 and one.residuals.max() > 1e-10 * one.bound
    assert np.all(np.isfinite(one.modes)) and one.bound == res.bound and res.converged
