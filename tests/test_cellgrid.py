"""The shared float32 cell grid (pesto_amd/csrc/pesto_cellgrid.h) through both of its users on ONE batch: pesto_interface_labels
(evaluate.contact_labels) and pesto_contacts (dataset._contacts_call), from host arrays and from ROCm tensors, against a NumPy float64
brute force. Four assemblies of two subunits each, r_thr = 5, the smallest shapes at which the grid's branches differ:
    a  2 atoms, one per subunit, 3 A apart                   one cell
    b  40 atoms uniform in a 60 A cube                       12^3 cells at the r_thr edge > 2 N + 64: the edge grows (h *= 1.25f)
    c  300 atoms in a 4 x 4 x 200 A rod                      nx = ny = 1, 40 cells along z, the clamps at the border
    d  64 atoms in a 12 A cube, one with a NaN coordinate    that atom has no contact and no label and gives none
(The bounding box is made with fminf / fmaxf, which pass over a NaN, so d's grid is an ordinary one that holds an atom no comparison is
true for; an INFINITE coordinate is what makes the box non-finite and the grid fall back to one cell: the last test.)
No brute-force distance lies within 1e-3 of r_thr (asserted without a GPU), so float32 rounding decides no pair and no tie flag is set."""
import numpy as np
import pytest

R_THR = 5.0
SEED = 3
RES_ATOMS = 3          # atoms per residue
BAD_ATOM = 30          # of assembly d: the last atom of its first subunit, a residue of its own


def _assemblies(seed=SEED, bad=np.nan):
    """[(xyz float32 [n, 3], atoms of the first subunit)] of a .. d"""
    rng = np.random.default_rng(seed)
    a = np.array([[0, 0, 0], [3, 0, 0]], np.float32) + np.float32(7.5)
    b = (rng.uniform(0, 60, (40, 3)) + [100, -50, 30]).astype(np.float32)
    c = (rng.uniform(0, 1, (300, 3)) * [4, 4, 200] - [2, 2, 100]).astype(np.float32)
    d = (rng.uniform(0, 12, (64, 3)) - [40, 0, 0]).astype(np.float32)
    d[BAD_ATOM, 1] = bad
    return [(a, 1), (b, 20), (c, 150), (d, BAD_ATOM + 1)]


def _brute_force(asm):
    """(pairs int64 [K, 2] of batch atom indices in the reference's order - per assembly, a then b ascending -, float64 distances [K],
    the smallest | distance - r_thr | over every pair of two subunits of an assembly, contacts per assembly)"""
    pairs, dist, margin, base, per = [], [], np.inf, 0, []
    for xyz, n0 in asm:
        x = xyz.astype(np.float64)
        D = np.sqrt(((x[:n0, None, :] - x[None, n0:, :]) ** 2).sum(-1))
        margin = min(margin, float(np.nanmin(np.abs(D - R_THR))))
        ia, ib = np.where(D < R_THR)                        # row-major: a, then b ascending; a NaN compares false
        pairs.append(np.stack([ia + base, ib + base + n0], 1))
        dist.append(D[ia, ib])
        per.append(ia.size)
        base += xyz.shape[0]
    return np.concatenate(pairs).astype(np.int64), np.concatenate(dist), margin, per


def _atom_residues(asm):
    """batch residue index of every atom (RES_ATOMS consecutive atoms of a subunit form a residue), the residue count"""
    res, r_base = [], 0
    for xyz, n0 in asm:
        for n in (n0, xyz.shape[0] - n0):
            res.append(np.arange(n) // RES_ATOMS + r_base)
            r_base += (n + RES_ATOMS - 1) // RES_ATOMS
    return np.concatenate(res).astype(np.int32), r_base


def _bad_atom(asm):
    return sum(a[0].shape[0] for a in asm[:3]) + BAD_ATOM


def test_no_distance_near_threshold():
    """the premise of the GPU tests below (runs without a GPU): the margin, and contacts where the cases are meant to have some"""
    asm = _assemblies()
    pairs, _, margin, per = _brute_force(asm)
    assert margin > 1e-3, margin
    assert per[0] == 1 and min(per[1:]) >= 1, per
    assert not np.any(pairs == _bad_atom(asm)) and BAD_ATOM % RES_ATOMS == 0
    assert np.isnan(asm[3][0]).sum() == 1


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


def _run(model, asm, on_device):
    """both users on the batch: (pairs, d, contact ties, labels, label ties) as host arrays"""
    import torch
    from pesto_amd import _lib, dataset, evaluate
    rows, sub, k = [], [], 0
    for xyz, n0 in asm:
        parts = [(f"s{k}", xyz[:n0]), (f"s{k + 1}", xyz[n0:])]
        rows.append([(nm, x, (np.arange(x.shape[0]) // RES_ATOMS).astype(np.int32), np.full(x.shape[0], -1, np.int32),
                      (x.shape[0] + RES_ATOMS - 1) // RES_ATOMS) for nm, x in parts])
        sub += [np.full(n0, k, np.int32), np.full(xyz.shape[0] - n0, k + 1, np.int32)]
        k += 2
    out, _ = dataset._contacts_call(model, rows, R_THR, dataset.MOLECULE_IDS, on_device)
    X = np.concatenate([a[0] for a in asm])
    res, n_res = _atom_residues(asm)
    if on_device:
        assert out["pairs"].is_cuda and out["d"].is_cuda
        X = torch.from_numpy(X).to("cuda:0")
    labels, lties = evaluate.contact_labels(model, X, np.concatenate(sub), res, np.ones(res.size, np.uint8), np.ones(res.size, np.uint32),
                                            [a[0].shape[0] for a in asm], n_res, R_THR)
    pairs, d, cties, labels, lties = (_lib.host(v) for v in (out["pairs"], out["d"], out["ties"], labels, lties))
    return pairs, d, cties, labels.view(np.uint32), lties           # (a device call returns the labels as the int32 of the same bits)


def _check(asm, got):
    pairs, d, cties, labels, lties = got
    want, want_d, _, _ = _brute_force(asm)
    np.testing.assert_array_equal(pairs.astype(np.int64), want)
    # float32 coordinates below 256 in size: each difference is off by at most 2^-24 * 256, the chain's own roundings are smaller still
    np.testing.assert_allclose(d.astype(np.float64), want_d, rtol=0, atol=1e-4)
    res, n_res = _atom_residues(asm)
    want_res = np.zeros(n_res, bool)
    want_res[res[want.reshape(-1)]] = True
    np.testing.assert_array_equal(labels != 0, want_res)
    assert set(np.unique(labels)) <= {0, 1}
    assert not cties.any() and not lties.any()


@pytest.fixture(scope="module")
def host_and_device(model):
    asm = _assemblies()
    return asm, _run(model, asm, False), _run(model, asm, True)


@pytest.mark.gpu
@pytest.mark.parametrize("side", [0, 1], ids=["host", "device"])
def test_pairs_and_labels_match_brute_force(host_and_device, side):
    asm = host_and_device[0]
    assert _brute_force(asm)[2] > 1e-3
    _check(asm, host_and_device[1 + side])
    pairs, _, _, labels, _ = host_and_device[1 + side]
    bad = _bad_atom(asm)                                     # the NaN atom: in no pair, its residue (it alone) not labelled
    assert not np.any(pairs == bad) and labels[_atom_residues(asm)[0][bad]] == 0


@pytest.mark.gpu
def test_host_and_device_identical_bits(host_and_device):
    _, host, dev = host_and_device
    for h, d in zip(host, dev):
        assert h.dtype == d.dtype and h.shape == d.shape and h.tobytes() == d.tobytes()


@pytest.mark.gpu
def test_infinite_coordinate_takes_the_one_cell_grid(model):
    """assembly d alone with an infinite coordinate: the bounding box is not finite, every pair is examined, the answer is the same"""
    asm = _assemblies(bad=np.inf)[3:]
    assert _brute_force(asm)[2] > 1e-3
    _check(asm, _run(model, asm, False))
