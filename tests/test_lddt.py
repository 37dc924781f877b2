"""GPU tests of pesto_amd.lddt (pesto_lddt.hip) against the NumPy definitions of test_lddt_fixture.py, through host arrays and ROCm
tensors. Everything is compared by equality: preserved, total and n_pairs as integers, score and residue as bits (NaN where the
definition has NaN), reference_pairs as arrays. A seeded sweep at the edges of the wave and of its four chunks in flight (rows of 0, 1, 63, 64, 65, 129, 255, 256 and 257 entries), of the
workgroup's four waves (R of 1, 3, 4, 5), of the frames (F of 1, 2, 65) and of the grid kernels' 256 threads (N of 2, 255, 256, 257);
the hand-worked cases with their ties; the recorded interface; invariances; missing atoms; the ragged batch; pairs= reuse; identical
bits from call to call and between the two sides; refused calls, which write nothing; more items than one launch holds; structure_lddt."""
import functools

import numpy as np
import pytest

from test_lddt_fixture import (DEFAULT_T, LATTICE_ALL, LATTICE_INTER, LATTICE_INTRA, hub_system, iface, iface_def, lattice, lddt_def, pairs_def,
                               perturbed_1thf, random_system)

pytestmark = pytest.mark.gpu

T8 = (0.25, 0.5, 1, 1.5, 2, 3, 4, 8)
# (system, its arguments, mode, thresholds, sel): rows of {0, 1, 63, 64, 65, 129, 255, 256, 257} entries and residues of 1 and 70 atoms (hub); R of
# {1, 3, 4, 5}; F of {1, 2, 65}; N of {2, 255, 256, 257}; T of {1, 4, 8}; the three modes; a contiguous, a strided and a permuted sel;
# res_of_atom dealt at random (random_system), so no residue's atoms are adjacent
SWEEP = [
    ("hub", dict(F=2), "all", DEFAULT_T, None),
    ("hub", dict(F=2), "inter", (1.0,), None),
    ("hub", dict(F=1), "intra", T8, None),
    ("hub", dict(F=65), "all", (2.0,), "strided"),
    ("rand", dict(N=2, R=1, F=1), "all", DEFAULT_T, None),
    ("rand", dict(N=2, R=2, F=2), "all", DEFAULT_T, None),
    ("rand", dict(N=255, R=3, F=65, nan_atoms=9), "all", (0.5,), "strided"),
    ("rand", dict(N=256, R=4, F=2), "inter", DEFAULT_T, "contiguous"),
    ("rand", dict(N=257, R=5, F=2, nan_atoms=9), "all", T8, "permuted"),
    ("rand", dict(N=257, R=4, F=1), "intra", DEFAULT_T, None),
    ("rand", dict(N=255, R=5, F=65), "inter", DEFAULT_T, "permuted"),
    ("rand", dict(N=256, R=1, F=2), "all", DEFAULT_T, None),
]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_result(a, b):
    return all(same_bits(getattr(a, k), getattr(b, k)) for k in ("score", "residue", "preserved", "total")) and np.array_equal(a.n_pairs, b.n_pairs)


def floats_equal(got, want):
    """the same float32 bits, NaN exactly where the definition has NaN"""
    got, want = host(got), np.asarray(want)
    assert got.dtype == np.float32 and want.dtype == np.float32 and got.shape == want.shape
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(got[~nan].view(np.uint32), want[~nan].view(np.uint32))


def check(out, want, on_device, tag=""):
    for key, dt in (("score", np.float32), ("residue", np.float32), ("preserved", np.int32), ("total", np.int32)):
        v = getattr(out, key)
        assert (v.is_cuda if on_device else isinstance(v, np.ndarray)) and host(v).dtype == dt, (tag, key)
    assert np.array_equal(out.n_pairs, want["n_pairs"]), tag
    assert np.array_equal(host(out.total), want["total"]), tag
    assert host(out.preserved).shape == want["preserved"].shape and np.array_equal(host(out.preserved), want["preserved"]), tag
    assert floats_equal(out.residue, want["residue"]), tag
    assert floats_equal(out.score, want["score"]), tag


def selection(kind, N, seed):
    if kind is None:
        return None
    if kind == "contiguous":
        return np.arange(N // 4, 3 * N // 4)
    if kind == "strided":
        m = np.zeros(N, bool)
        m[::3] = True
        m[1::7] = True
        return m
    return np.random.default_rng(seed).permutation(N)[:2 * N // 3]


@functools.lru_cache(maxsize=None)
def sweep_case(k):
    """(system, sel, the definition's pairs and result) of SWEEP[k], made once"""
    kind, kw, mode, thr, sk = SWEEP[k]
    s = hub_system(100 + k, **kw) if kind == "hub" else random_system(100 + k, **kw)
    sel = selection(sk, s["ref"].shape[0], k)
    pairs = pairs_def(s["ref"], s["roa"], s["chain"], mode, sel, 15.0, 1.0)
    return s, sel, pairs, lddt_def(s["ref"], s["xyz"], s["roa"], s["chain"], mode, sel, thr, 15.0, 1.0, pairs=pairs)


@pytest.mark.parametrize("k", range(len(SWEEP)), ids=lambda k: "%s-%s-%s-T%d" % (SWEEP[k][0], "-".join(f"{a}{b}" for a, b in SWEEP[k][1].items()),
                                                                                   SWEEP[k][2], len(SWEEP[k][3])))
def test_seeded_sweep(k):
    from pesto_amd import lddt as L
    _, kw, mode, thr, _ = SWEEP[k]
    s, sel, pairs, want = sweep_case(k)
    if SWEEP[k][0] == "hub":
        rows = set(np.diff(pairs_def(s["ref"], s["roa"], scale=1.0)[0]).tolist())
        assert {0, 1, 63, 64, 65, 129, 255, 256, 257} <= rows and np.bincount(s["roa"]).max() == 70 and np.bincount(s["roa"]).min() == 1
    else:
        assert s["ref"].shape[0] == kw["N"] and int(s["roa"].max()) + 1 == kw["R"] and (kw["N"] < 200 or kw["R"] == 1 or np.any(np.diff(s["roa"]) < 0))
    assert s["xyz"].shape[0] == kw["F"] and want["preserved"].shape[2] == len(thr)
    for on_device in (False, True):
        ref, xyz = (dev(s["ref"]), dev(s["xyz"])) if on_device else (s["ref"], s["xyz"])
        out = L.lddt(ref, xyz, s["roa"], s["chain"], mode, sel, thr, 15.0, 1.0)
        check(out, want, on_device, k)
        got = L.reference_pairs(ref, s["roa"], s["chain"], mode, sel, 15.0, 1.0)
        assert all((v.is_cuda if on_device else isinstance(v, np.ndarray)) for v in got)
        assert host(got[0]).dtype == np.int64 and host(got[1]).dtype == np.int32 and host(got[2]).dtype == np.float32
        assert np.array_equal(host(got[0]), pairs[0]) and np.array_equal(host(got[1]), pairs[1]) and same_bits(got[2], pairs[2])
    if want["n_pairs"]:
        assert np.all(host(out.residue)[0][want["total"] > 0] == 1.0) and host(out.score)[0] == 1.0            # frame 0 is the reference
    else:
        assert np.isnan(host(out.score)).all() and np.isnan(host(out.residue)).all()


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_hand_worked_cases(on_device):
    from pesto_amd import lddt as L
    s = lattice()
    ref, xyz = (dev(s["ref"]), dev(s["xyz"])) if on_device else (s["ref"], s["xyz"])
    out = L.lddt(ref, xyz, s["roa"], scale=1.0)
    assert out.n_pairs == 8 and host(out.total).tolist() == LATTICE_ALL["total"] and host(out.preserved).tolist() == LATTICE_ALL["preserved"]
    assert floats_equal(out.residue, np.array(LATTICE_ALL["residue"], np.float32)) and floats_equal(out.score, np.array(LATTICE_ALL["score"], np.float32))
    check(out, lddt_def(s["ref"], s["xyz"], s["roa"], scale=1.0), on_device)
    off, j, d = (host(v) for v in L.reference_pairs(ref, s["roa"], scale=1.0))
    assert off.tolist() == LATTICE_ALL["offsets"] and j.tolist() == LATTICE_ALL["j"] and d[0] == 3 and d[5] == 5      # (0, 1) at exactly 15 is out
    assert host(L.reference_pairs(ref, s["roa"], r_incl=float(np.nextafter(np.float32(15), np.float32(16))), scale=1.0)[0])[-1] == 10
    for fn, want in ((lambda **kw: L.ilddt(ref, xyz, s["roa"], s["chain"], scale=1.0, **kw), LATTICE_INTER),
                     (lambda **kw: L.lddt(ref, xyz, s["roa"], s["chain"], "intra", scale=1.0, **kw), LATTICE_INTRA)):
        got = fn()
        assert got.n_pairs == want["n_pairs"] and host(got.total).tolist() == want["total"]
    assert host(L.ilddt(ref, xyz, s["roa"], s["chain"], scale=1.0).preserved)[1].tolist() == [[0, 1, 2, 2], [1, 1, 1, 1], [1, 2, 3, 3], [0, 0, 0, 0]]
    check(L.ilddt(ref, xyz, s["roa"], s["chain"], scale=1.0), lddt_def(s["ref"], s["xyz"], s["roa"], s["chain"], "inter", scale=1.0), on_device)
    # the same poses read as nanometres
    ten = L.lddt(ref, xyz, s["roa"], r_incl=150.0, thresholds=(5, 10, 20, 40), scale=10.0)
    assert host(ten.preserved).tolist() == LATTICE_ALL["preserved"]


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_recorded_interface(on_device):
    from pesto_amd import lddt as L
    s = iface()
    xyz = dev(s["xyz"]) if on_device else s["xyz"]
    out = L.lddt(xyz[0], xyz, s["roa"])
    check(out, iface_def(), on_device)
    assert out.n_pairs == 505876 and host(out.score)[0] == 1.0 and 0.685 <= host(out.score).min() < 0.695
    check(L.ilddt(xyz[0], xyz, s["roa"], s["chain"]), iface_def("inter"), on_device)
    check(L.lddt_ca(xyz[0], xyz, s["roa"], s["ca"]), iface_def("all", True), on_device)
    if not on_device:
        off, j, d = L.reference_pairs(xyz[0], s["roa"])
        want = pairs_def(s["xyz"][0], s["roa"])
        assert np.array_equal(off, want[0]) and np.array_equal(j, want[1]) and same_bits(d, want[2])


def test_invariances():
    from pesto_amd import lddt as L
    s = random_system(7, 300, 40, 3)
    rng = np.random.default_rng(7)
    same = L.lddt(s["ref"], s["ref"], s["roa"], scale=1.0)
    assert np.all(host(same.residue)[0][host(same.total) > 0] == 1.0) and host(same.score)[0] == 1.0 and (host(same.total) > 0).any()
    # a rigid motion of the frames: the distances are recomputed from rounded coordinates, so the definition on the MOVED frames decides
    q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    moved = (s["xyz"].astype(np.float64) @ q + np.array([3.0, -20.0, 11.0])).astype(np.float32)
    out = L.lddt(s["ref"], moved, s["roa"], scale=1.0)
    check(out, lddt_def(s["ref"], moved, s["roa"], scale=1.0), False)
    still = L.lddt(s["ref"], s["xyz"], s["roa"], scale=1.0)
    # a frame blown up by 2 keeps fewer distances
    big = L.lddt(s["ref"], s["xyz"] * np.float32(2), s["roa"], scale=1.0)
    check(big, lddt_def(s["ref"], s["xyz"] * np.float32(2), s["roa"], scale=1.0), False)
    assert np.all(host(big.preserved).sum((1, 2)) < host(still.preserved).sum((1, 2))) and np.all(host(big.score) < host(still.score))


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_missing_atoms(on_device):
    from pesto_amd import lddt as L
    s = random_system(11, 200, 30, 4)
    rng = np.random.default_rng(11)
    xyz = s["xyz"].copy()
    xyz[1, rng.choice(200, 40, replace=False)] = np.nan          # atoms missing in a frame
    xyz[2, :, 0] = np.nan                                        # one coordinate of every atom
    xyz[3] = np.nan                                              # a frame without any atom
    ref = s["ref"].copy()
    ref[rng.choice(200, 25, replace=False), rng.integers(0, 3, 25)] = np.nan          # atoms missing in the reference
    ref[5] = np.inf
    for y in (s["ref"], ref):
        want = lddt_def(y, xyz, s["roa"], scale=1.0)
        out = L.lddt(dev(y) if on_device else y, dev(xyz) if on_device else xyz, s["roa"], scale=1.0)
        check(out, want, on_device)
        assert host(out.score)[2] == 0 and host(out.score)[3] == 0 and host(out.preserved)[2:].sum() == 0 and 0 < host(out.score)[1] < 1
    assert want["n_pairs"] < lddt_def(s["ref"], xyz[:1], s["roa"], scale=1.0)["n_pairs"]
    # a reference without any finite atom: no pair, every score NaN
    out = L.lddt(np.full_like(ref, np.nan), xyz, s["roa"], scale=1.0)
    assert out.n_pairs == 0 and np.isnan(host(out.score)).all() and host(out.total).sum() == 0


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_ragged_batch(on_device):
    from pesto_amd import lddt as L
    parts = [random_system(21, 5, 1, 2), random_system(22, 257, 9, 2, nan_atoms=5), random_system(23, 64, 4, 2), random_system(24, 30, 3, 2)]
    parts[3]["ref"][:] = np.nan                                   # a structure whose reference has no coordinates at all
    parts[2]["ref"][3, 1] = np.nan                                # and one that lacks an atom
    sizes = [p["ref"].shape[0] for p in parts]
    ref = np.concatenate([p["ref"] for p in parts])
    xyz = np.concatenate([p["xyz"][1] for p in parts])
    starts = np.cumsum([0] + [int(p["roa"].max()) + 1 for p in parts])
    roa = np.concatenate([p["roa"] + starts[b] for b, p in enumerate(parts)])
    chain = np.concatenate([p["chain"] for p in parts])
    put = dev if on_device else (lambda a: a)
    for mode in ("all", "inter"):
        out = L.lddt(put(ref), put(xyz), roa, chain, mode, scale=1.0, sizes=sizes)
        check(out, lddt_def(ref, xyz, roa, chain, mode, scale=1.0, sizes=sizes), on_device, mode)
        assert host(out.score).shape == (4,) and np.isnan(host(out.score)[0]) and np.isnan(host(out.score)[3]) and out.n_pairs[0] == 0
        for b, p in enumerate(parts):
            one = L.lddt(put(p["ref"]), put(p["xyz"][1]), p["roa"], p["chain"], mode, scale=1.0)
            assert one.n_pairs == out.n_pairs[b] and same_bits(host(one.score), host(out.score)[b:b + 1])
            assert same_bits(host(one.residue), host(out.residue)[:, starts[b]:starts[b + 1]])
            assert same_bits(host(one.preserved), host(out.preserved)[:, starts[b]:starts[b + 1]])
            assert same_bits(host(one.total), host(out.total)[starts[b]:starts[b + 1]])
    got = L.reference_pairs(put(ref), roa, sizes=sizes, scale=1.0)
    want = pairs_def(ref, roa, scale=1.0, sizes=sizes)
    assert np.array_equal(host(got[0]), want[0]) and np.array_equal(host(got[1]), want[1]) and same_bits(got[2], want[2])


def test_pairs_reuse_and_repeatability():
    from pesto_amd import lddt as L
    s = hub_system(31, F=9)
    sel = selection("strided", s["ref"].shape[0], 0)
    args = (s["roa"], s["chain"], "inter", sel, T8, 15.0, 1.0)
    first = L.lddt(s["ref"], s["xyz"], *args)
    check(first, lddt_def(s["ref"], s["xyz"], *args), False)
    assert same_result(first, L.lddt(s["ref"], s["xyz"], *args))                                      # from call to call
    on_dev = L.lddt(dev(s["ref"]), dev(s["xyz"]), *args)
    assert same_result(first, on_dev) and same_result(on_dev, L.lddt(dev(s["ref"]), dev(s["xyz"]), *args))         # between the sides
    for put in (lambda a: a, dev):
        pairs = L.reference_pairs(put(s["ref"]), s["roa"], s["chain"], "inter", sel, 15.0, 1.0)
        again = L.lddt(put(s["ref"]), put(s["xyz"]), s["roa"], thresholds=T8, scale=1.0, pairs=pairs)         # mode and sel live in the list
        assert same_result(first, again)
        assert same_bits(pairs[1], L.reference_pairs(put(s["ref"]), s["roa"], s["chain"], "inter", sel, 15.0, 1.0)[1])
    mixed = L.lddt(dev(s["ref"]), dev(s["xyz"]), s["roa"], thresholds=T8, scale=1.0, pairs=tuple(host(v) for v in pairs))
    assert same_result(first, mixed)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_a_refused_call_writes_nothing(on_device, monkeypatch):
    import torch
    from pesto_amd import _lib
    from pesto_amd import lddt as L
    s = lattice()
    off, j, d = pairs_def(s["ref"], s["roa"], scale=1.0)
    made = []
    plain = _lib.Side.empty

    def filled(self, shape, dtype):
        a = plain(self, shape, dtype)
        if self.device is None:
            a.view(np.uint8)[...] = 0xA5
        else:
            a.view(torch.uint8).fill_(0xA5)
        made.append(a)
        return a
    monkeypatch.setattr(_lib.Side, "empty", filled)
    ref, xyz = (dev(s["ref"]), dev(s["xyz"])) if on_device else (s["ref"], s["xyz"])
    bad_j, bad_off, neg = j.copy(), off.copy(), off.copy()
    bad_j[3] = 5                                                 # a partner outside [0, N)
    bad_off[2] = 7                                               # offsets that run backwards
    neg[0] = -1
    for pairs, word in (((off, bad_j, d), "partners"), ((bad_off, j, d), "offsets"), ((neg, j, d), "offsets"), ((off + 1, j, d), "offsets")):
        made.clear()
        with pytest.raises(_lib.PestoError, match=word):
            L.lddt(ref, xyz, s["roa"], scale=1.0, pairs=pairs)
        assert len(made) == 4
        for a in made:                                           # score, residue, preserved, total: as they were
            assert (host(a).view(np.uint8) == 0xA5).all()
    monkeypatch.setattr(_lib.Side, "empty", plain)
    out = L.lddt(ref, xyz, s["roa"], scale=1.0, pairs=(off, j, d))          # the same call with the list as it should be
    assert host(out.preserved).tolist() == LATTICE_ALL["preserved"]


def test_more_items_than_the_launch_holds():
    """F * ceil(R / 4) = (2^18 + 1) * 5 items, beyond the 2^20 workgroups of the scoring launch: every workgroup strides over several
    items. The frames repeat three distinct ones, so the definition of those three, repeated, is the definition of all."""
    from pesto_amd import lddt as L
    s = random_system(41, 17, 17, 3, box=12.0, nan_atoms=2)
    F = 2 ** 18 + 1
    want = lddt_def(s["ref"], s["xyz"], s["roa"], thresholds=(1.0,), scale=1.0)
    assert want["n_pairs"] > 100 and len(set(want["score"].tolist())) == 3 and F * -(-17 // 4) > 2 ** 20
    which = np.arange(F) % 3
    out = L.lddt(dev(s["ref"]), dev(s["xyz"])[dev(which)], s["roa"], thresholds=(1.0,), scale=1.0)
    assert out.n_pairs == want["n_pairs"] and np.array_equal(host(out.total), want["total"])
    assert np.array_equal(host(out.preserved), want["preserved"][which])
    assert floats_equal(out.residue, want["residue"][which]) and floats_equal(out.score, want["score"][which])


def test_structure_lddt_on_1thf():
    from pesto_amd import lddt as L
    ref, model, gone, _ = perturbed_1thf()
    y, x, res, chain, table = L.match_atoms(ref, model)
    out, tab = L.structure_lddt(ref, model)
    check(out, lddt_def(y, x, res, chain, scale=1.0), False)
    row = int(np.nonzero((tab["chain_name"] == gone[0]) & (tab["resid"] == gone[1]))[0][0])
    assert host(out.residue)[0, row] == 0 and 0.3 < host(out.score)[0] < 1 and host(out.residue).shape == (1, len(tab["resid"]))
    ca, _ = L.structure_lddt(ref, model, ca_only=True)
    check(ca, lddt_def(y, x, res, chain, sel=ref["name"] == "CA", scale=1.0), False)
    assert 0 < ca.n_pairs < out.n_pairs
