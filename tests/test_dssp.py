"""GPU tests of pesto_amd.dssp (pesto_dssp.hip) against the definition's golden (tests/golden/dssp.npz): codes, partners and the energies
in thousandths equal element for element - through host arrays and ROCm tensors, the batch in one launch, one structure at a time and
reversed, all frames in one call and frame by frame, every planted case (the residue counts around the kernel's LDS tile of 128 and its
workgroup of 256 among them), two runs, scale=10 on float32(X / 10) (codes only, on the structures the generator checked), the reader's
dicts through structure_dssp, and Model.forward_frames followed by compute_dssp on the same device tensor."""
import numpy as np
import pytest

from conftest import golden, md_frames, weights
from test_dssp_fixture import batch_dicts, case, planted_names

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def run(X, table, sizes, scale=1.0, model=None):
    """(codes, partners, e_m) as the golden stores them"""
    from pesto_amd import dssp as DS
    codes = DS.compute_dssp(X, table, sizes=sizes, scale=scale, model=model, return_codes=True)
    partners, energies = DS.kabsch_sander(X, table, sizes=sizes, scale=scale, model=model)
    assert host(energies).dtype == np.float32
    return host(codes), host(partners), np.rint(host(energies).astype(np.float64) * 1000.0).astype(np.int32)


def check(got, want, what):
    for g, w, name in zip(got, want, ("codes", "partners", "e_m")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, (what, name, bad[:5].tolist(), g[tuple(bad[0])], w[tuple(bad[0])])


def split_batch(g):
    """[(X, table tuple, codes, partners, e_m)] of the batch's structures, each with atom rows of its own"""
    X, (table, pro, chain), sizes, codes, partners, em = case(g, "batch")
    out, r0 = [], 0
    for n in sizes:
        t = table[r0:r0 + n]
        lo, hi = int(t[t >= 0].min()), int(t.max()) + 1
        out.append((X[:, lo:hi], (np.where(t >= 0, t - lo, -1).astype(np.int32), pro[r0:r0 + n], chain[r0:r0 + n]), codes[:, r0:r0 + n],
                    partners[:, r0:r0 + n], em[:, r0:r0 + n]))
        r0 += n
    return out


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_batch_in_one_launch(on_device):
    from pesto_amd import dssp as DS
    g = golden("dssp")
    X, table, sizes, codes, partners, em = case(g, "batch")
    x = dev(X) if on_device else X
    c = DS.compute_dssp(x, table, sizes=sizes, return_codes=True)
    p, e = DS.kabsch_sander(x, table, sizes=sizes)
    assert (c.is_cuda and p.is_cuda and e.is_cuda) if on_device else all(isinstance(a, np.ndarray) for a in (c, p, e))
    check(run(x, table, sizes), (codes, partners, em), "batch")
    if on_device:
        assert DS.compute_dssp(x, table, sizes=sizes).is_cuda                      # a ROCm tensor in: the uint8 codes as a tensor
    else:
        full = DS.compute_dssp(X, table, simplified=False, sizes=sizes)
        assert full.dtype == np.dtype("<U2") and np.array_equal(full, DS.letters(codes, simplified=False))
        assert np.array_equal(DS.compute_dssp(X, table, sizes=sizes), DS.letters(codes))
        one = DS.compute_dssp(X[0], table, sizes=sizes)
        assert one.shape == (codes.shape[1],) and np.array_equal(one, DS.letters(codes[0]))


def test_one_structure_at_a_time_and_the_batch_reversed():
    g = golden("dssp")
    parts = split_batch(g)
    for k, (X, table, codes, partners, em) in enumerate(parts):
        check(run(X, table, None), (codes, partners, em), f"structure {k}")
    rev = parts[::-1]
    atoms = np.cumsum([0] + [p[0].shape[1] for p in rev])
    table = (np.concatenate([np.where(p[1][0] >= 0, p[1][0] + a, -1) for p, a in zip(rev, atoms)]).astype(np.int32),
             np.concatenate([p[1][1] for p in rev]), np.concatenate([p[1][2] for p in rev]))
    got = run(np.concatenate([p[0] for p in rev], 1), table, [p[2].shape[1] for p in rev])
    check(got, tuple(np.concatenate([p[k] for p in rev], 1) for k in (2, 3, 4)), "reversed batch")


def test_reader_dicts_through_structure_dssp():
    from pesto_amd import dssp as DS
    g = golden("dssp")
    dicts = batch_dicts(g)
    many = DS.structure_dssp(dicts)
    parts = split_batch(g)
    assert len(many) == len(parts)
    for d, ss, (_, _, codes, _, _) in zip(dicts, many, parts):
        keep = (DS.backbone_table(d)[0] >= 0).any(1)                  # the golden holds the residues with a backbone atom
        assert ss.shape == (1, keep.size) and (ss[0][~keep] == "NA").all()
        assert np.array_equal(ss[0][keep], DS.letters(codes[0], simplified=False))
    assert np.array_equal(DS.structure_dssp(dicts[2]), many[2])


def test_all_frames_in_one_call_and_frame_by_frame():
    g = golden("dssp")
    X, table, sizes, codes, partners, em = case(g, "frames")
    assert X.shape[0] == 8
    check(run(X, table, sizes), (codes, partners, em), "frames")
    check(run(dev(X), table, sizes), (codes, partners, em), "frames on the device")
    for f in range(X.shape[0]):
        got = run(X[f], table, sizes)
        check(got, (codes[f], partners[f], em[f]), f"frame {f}")


def test_every_planted_case():
    g = golden("dssp")
    for name in planted_names(g):
        X, table, sizes, codes, partners, em = case(g, "planted_" + name)
        check(run(X, table, sizes), (codes, partners, em), name)
        check(run(dev(X), table, sizes), (codes, partners, em), name + " on the device")


def test_two_runs_give_identical_bits():
    g = golden("dssp")
    X, table, sizes, _, _, _ = case(g, "batch")
    x = dev(X)
    a, b = run(x, table, sizes), run(x, table, sizes)
    assert all(np.array_equal(u, v) for u, v in zip(a, b))


def test_scale_10_on_coordinates_divided_by_10():
    from pesto_amd import dssp as DS
    g = golden("dssp")
    _, table, sizes, codes, _, _ = case(g, "batch")
    got = DS.compute_dssp(g["scale10_X"], table, sizes=sizes, scale=10.0, return_codes=True)
    cuts = np.cumsum([0] + sizes)
    for k in g["scale10_ok"].tolist():                                # the structures the generator checked to stay unflagged
        assert np.array_equal(got[cuts[k]:cuts[k + 1]], codes[0][cuts[k]:cuts[k + 1]]), k


def test_forward_frames_then_dssp_on_the_same_device_tensor():
    import torch
    from pesto_amd import Model
    from pesto_amd import dssp as DS
    from pesto_amd.config import CONFIGS
    f = md_frames()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), dev(f["res_of_atom"]).long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    # the fixture holds no atom names: a table over the first four atoms of every residue exercises the call, not the chemistry
    roa = f["res_of_atom"]
    assert (np.diff(roa) >= 0).all()
    first = np.searchsorted(roa, np.arange(f["R"]))
    count = np.bincount(roa, minlength=f["R"])
    table = np.where(np.arange(4)[None, :] < count[:, None], first[:, None] + np.arange(4)[None, :], -1).astype(np.int32)
    codes = DS.compute_dssp(X, table, model=m)
    on_host = DS.compute_dssp(f["X_frames"], table, return_codes=True)
    assert z.is_cuda and codes.is_cuda and codes.dtype == torch.uint8 and tuple(codes.shape) == (X.shape[0], f["R"])
    assert np.abs(host(z) - f["z"]).max() < 1e-4
    assert np.array_equal(host(codes), on_host) and ((on_host == 8) == (count < 4)[None]).all()
