"""GPU tests of what the call helpers own (pesto_call.h: cleared buffers and Buffers::verdict; pesto_scan.h: list_scan, list_offsets and
list_tail), through the smallest inputs that reach every branch of them, on the host side and on the device side:
  - the list-valued wrappers with a ``capacity=`` argument at capacities 1, K - 1, K and K + 1 and on an input with an empty list: the
    refill path, the exact fit and the empty fetch all give the lists of the generous call bit for bit;
  - one refused call per way an entry point reads the device's verdict: the library's message word for word, the outputs untouched where
    the group promises that, and a valid call on the same handle straight afterwards;
  - an output that the declaration clears, as a caller-owned tensor on the device side.
The entry points are called through the C ABI where the Python layer would refuse the argument first."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIDES = pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


def placer(on_device):
    return dev if on_device else np.ascontiguousarray


# ------------------------------------------------------------------ list-valued calls
def contacts_input(empty):
    """two frames of 5 x 4 atoms in a box of 5 A (nm, scale 10): most pairs are contacts; empty: side b 100 nm away"""
    rng = np.random.default_rng(5)
    xa = rng.uniform(0.0, 0.5, (2, 5, 3)).astype(np.float32)
    xb = rng.uniform(0.0, 0.5, (2, 4, 3)).astype(np.float32)
    return xa, xb + np.float32(100.0 if empty else 0.0)


def hbonds_input(empty):
    """3 donor pairs x 4 acceptors on near-parallel lines, D - H 1 A, H .. A 2 A, the angle near 180 degrees: all 12 triplets are bonded
    in frame 0, the 6 of acceptors 0 and 1 in frame 1; empty: every acceptor 50 nm away"""
    xyz = np.zeros((2, 10, 3), np.float32)
    for p in range(3):
        xyz[:, 2 * p] = (0.0, 0.02 * p, 0.0)
        xyz[:, 2 * p + 1] = (0.1, 0.02 * p, 0.0)
    for a in range(4):
        xyz[:, 6 + a] = (0.3, 0.02 * a, 0.01 * a)
    xyz[1, 8:, 0] += 50.0
    if empty:
        xyz[:, 6:, 0] += 50.0
    return xyz, np.array([[0, 1], [2, 3], [4, 5]], np.int32), np.array([6, 7, 8, 9], np.int32)


def list_call(group, on_device, empty, capacity):
    """(offsets, rows, values...) of one wrapper call"""
    put = placer(on_device)
    if group == "docking":
        from pesto_amd import docking as D
        xa, xb = contacts_input(empty)
        return D.frame_contacts(put(xa), put(xb), capacity=capacity)
    if group == "hbonds":
        from pesto_amd import hbonds as H
        xyz, dh, acc = hbonds_input(empty)
        return H.frame_hbonds(put(xyz), dh, acc, capacity=capacity)
    from pesto_amd import ranking as R
    y = np.array([1, 0, 1, 1, 0, 0], np.uint8)
    p = np.array([0.9, 0.8, 0.8, 0.4, 0.3, 0.1], np.float32)            # five distinct thresholds
    return R.curves(put(y), put(p), capacity=capacity)


@SIDES
@pytest.mark.parametrize("group", ["docking", "hbonds", "ranking"])
def test_lists_are_the_same_at_every_capacity(group, on_device):
    want = list_call(group, on_device, False, None)
    K = int(host(want[0])[-1])
    assert K >= 3 and all(host(a).shape[0] == K for a in want[1:]), K
    if group == "hbonds":
        assert host(want[0]).tolist() == [0, 12, 18]
    for cap in (1, K - 1, K, K + 1):
        got = list_call(group, on_device, False, cap)
        assert all(same_bits(g, w) for g, w in zip(got, want)), cap            # (the offsets, and with them the reported size K)
        assert all((g.is_cuda if on_device else isinstance(g, np.ndarray)) for g in got[1:]), cap
    if group == "ranking":
        return                                                                  # (a column always has a threshold: K >= 1)
    for cap in (1, None):
        got = list_call(group, on_device, True, cap)
        assert not host(got[0]).any() and all(host(a).shape[0] == 0 for a in got[1:]), cap
    assert all(same_bits(g, w) for g, w in zip(list_call(group, on_device, False, K), want))         # and the handle is as before


def handle():
    from pesto_amd import _lib
    from pesto_amd.patches import _default_model
    model = _default_model(0)
    return model, _lib.load()


@SIDES
def test_a_list_that_does_not_fit_is_counted_and_not_brought_back(on_device):
    """the wrappers repeat such a call, so only the C ABI shows it: capacity 1 with arrays that could hold all K entries"""
    from pesto_amd import _lib
    from pesto_amd import docking as D
    model, lib = handle()
    put = placer(on_device)
    xa, xb = (put(a) for a in contacts_input(False))
    want = D.frame_contacts(xa, xb)
    K = int(host(want[0])[-1])
    side = _lib.Side(xa, model._gpu)
    offsets, pairs, d, sz = put(np.zeros(3, np.int64)), put(np.full((K, 2), 7, np.int32)), put(np.full(K, 7, np.float32)), np.zeros(1, np.int64)
    rc = lib.pesto_frame_contacts(model.handle, 2, 5, 4, side.ptr(xa), side.ptr(xb), 5.0, 10.0, 1, side.ptr(offsets), side.ptr(pairs), side.ptr(d),
                                  sz.ctypes.data, side.kind, side.stream)
    assert rc == 0 and int(sz[0]) == K >= 3 and same_bits(offsets, want[0])
    assert (host(pairs) == 7).all() and (host(d) == 7).all()


# ------------------------------------------------------------------ refused calls

def refused(lib, last_error, rc, text):
    """the library's message of a refused call, word for word as the entry point's source file has it"""
    from pesto_amd import _lib
    assert rc == -1
    with pytest.raises(_lib.PestoError) as e:
        _lib.check(rc, last_error)
    assert str(e.value) == "libpesto_hip error -1: " + text and e.value.code == -1


@SIDES
def test_fit_rmsd_refuses_an_index_and_serves_the_next_call(on_device):
    # (every selection and the sentinels of pesto_dockq itself: tests/test_dockq.py::test_a_refused_call_writes_nothing)
    from pesto_amd import _lib
    from pesto_amd import dockq as Q
    model, lib = handle()
    put = placer(on_device)
    xyz = np.random.default_rng(11).normal(size=(2, 5, 3)).astype(np.float32)
    x = put(xyz)
    side = _lib.Side(x, model._gpu)
    good, bad = np.array([0, 1, 2, 4], np.int32), np.array([0, 1, 2, 5], np.int32)
    out = put(np.full(2, 7, np.float32))

    def call(sel):
        s = put(sel)
        return lib.pesto_fit_rmsd(model.handle, 2, 1, 5, side.ptr(x), side.ptr(x), 4, side.ptr(s), 4, side.ptr(s), 1.0, side.ptr(out), side.kind,
                                  side.stream)
    refused(lib, lib.pesto_dockq_last_error, call(bad), "fit_rmsd: atom indices of a selection or of the permutation must lie in [0, N)")
    assert (host(out) == 7).all()                                               # pesto_amd.dockq: a refused call writes nothing
    assert call(good) == 0 and same_bits(out, Q.fit_rmsd(x[:1], x, good, good, scale=1.0))


@SIDES
def test_unwrap_pbc_refuses_a_permutation_and_serves_the_next_call(on_device):
    from pesto_amd import _lib
    from pesto_amd import hbonds as H
    model, lib = handle()
    put = placer(on_device)
    xyz = np.random.default_rng(13).uniform(0, 2, (1, 4, 3)).astype(np.float32)
    x, box, ms = put(xyz), put(np.full((1, 3), 2.0, np.float32)), put(np.ones(4, np.float64))
    side = _lib.Side(x, model._gpu)
    off = np.array([0, 2, 4], np.int32)
    out, image = put(np.zeros((1, 4, 3), np.float32)), put(np.zeros((1, 2), np.int32))

    def call(perm):
        p = put(np.array(perm, np.int32))
        return lib.pesto_unwrap_pbc(model.handle, 1, 4, 2, side.ptr(x), side.ptr(box), side.ptr(p), off.ctypes.data, side.ptr(ms), side.ptr(out),
                                    side.ptr(image), side.kind, side.stream)
    refused(lib, lib.pesto_hbonds_last_error, call([0, 1, 2, 4]), "perm: atom indices must lie in [0, N)")
    refused(lib, lib.pesto_hbonds_last_error, call([0, 1, 2, 2]), "perm: every atom must be named once (an index is repeated)")
    assert call([0, 1, 2, 3]) == 0
    assert same_bits(out, H.unwrap_pbc(x, box, np.array([0, 0, 1, 1]), masses=np.ones(4)))


@SIDES
def test_weighted_centers_refuses_a_weight_and_writes_nothing(on_device):
    # (the ValueError of the wrapper and its next call: tests/test_peaks.py; here the library's text and the caller's own arrays)
    from pesto_amd import _lib
    from pesto_amd import peaks as K
    model, lib = handle()
    put = placer(on_device)
    xp = put(np.random.default_rng(17).normal(size=(1, 2, 3)).astype(np.float32))
    side = _lib.Side(xp, model._gpu)
    outs = [put(np.full((1, 3), 7, np.float32)), put(np.full(1, 7, np.float64)), put(np.full(1, 7, np.float32))]

    def call(w):
        wd = put(np.array([w], np.float32))
        return lib.pesto_weighted_centers(model.handle, 1, 2, side.ptr(xp), side.ptr(wd), 1, 0.0, *(side.ptr(o) for o in outs), side.kind,
                                          side.stream)
    refused(lib, lib.pesto_peaks_last_error, call([1.0, -1.0]), "W has a negative or non-finite weight")
    assert all((host(o) == 7).all() for o in outs)
    assert call([1.0, 3.0]) == 0
    assert all(same_bits(o, w) for o, w in zip(outs, K.weighted_centers(xp, put(np.array([[1.0, 3.0]], np.float32)))))


@SIDES
def test_vertex_scores_refuses_an_atom_and_serves_the_next_call(on_device):
    from pesto_amd import _lib
    model, lib = handle()
    put = placer(on_device)
    p = put(np.array([0.25, 0.5], np.float32))
    side = _lib.Side(p, model._gpu)
    out = put(np.zeros(3, np.float32))

    def call(nearest):
        n = put(np.array(nearest, np.int32))
        return lib.pesto_surface_vertex_scores(model.handle, 3, 2, side.ptr(n), side.ptr(p), side.ptr(out), side.kind, side.stream)
    refused(lib, lib.pesto_surface_last_error, call([0, 5, 1]),
            "surface_vertex_scores: a nearest-atom index is neither -1 nor an atom of the vertex's structure")
    assert call([1, -1, 0]) == 0
    got = host(out)
    assert got[0] == 0.5 and np.isnan(got[1]) and got[2] == 0.25


# ------------------------------------------------------------------ cleared buffers
@SIDES
def test_areas_without_a_face_are_cleared_in_the_callers_own_array(on_device):
    from pesto_amd import _lib
    model, lib = handle()
    put = placer(on_device)
    v = put(np.random.default_rng(19).normal(size=(5, 3)).astype(np.float32))
    side = _lib.Side(v, model._gpu)
    vo, fo = np.array([0, 2, 5], np.int32), np.zeros(3, np.int32)               # two structures, five vertices, no face
    out = put(np.full(5, 0x0707070707070707, np.int64))
    assert lib.pesto_surface_areas(model.handle, 2, vo.ctypes.data, fo.ctypes.data, side.ptr(v), None, side.ptr(out), side.kind, side.stream) == 0
    assert not host(out).any()
