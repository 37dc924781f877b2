"""GPU tests of pesto_amd.sasa (pesto_sasa.hip) against the definition's golden (tests/golden/sasa.npz): counts equal bit for bit, areas
and residue sums equal as uint32 views the double-evaluated, once-rounded values - through host arrays and ROCm tensors, all frames in one
call and frame by frame, a ragged batch in one launch and one structure at a time, candidate lists longer than the LDS tile, every
planted case, a permutation of the atoms, two runs, buried_area on a two-chain assembly, and Model.forward_frames followed by sasa on the
same device tensor."""
import gzip
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden, md_frames, weights
from test_sasa_fixture import PROBE, areas_of, batch_structures, group_sums, planted_case, planted_names

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(a):
    return a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)


def same_bits(a, b):
    a, b = host(a), host(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def md_case():
    g, f = golden("sasa"), golden("frames_md_1JTG_uL")
    return f["X_frames"], g["md_R"], f["res_of_atom"].astype(np.int32), g["md_counts"].astype(np.int32)


@pytest.mark.parametrize("on_device", [False, True], ids=["host", "device"])
def test_md_counts_areas_and_residue_sums(on_device):
    from pesto_amd import sasa as SA
    X, R, roa, want = md_case()
    x, r = (dev(X), dev(R)) if on_device else (X, R)          # R holds the probe already: probe_radius=0 adds nothing
    area, counts = SA.shrake_rupley(x, radii=r, probe_radius=0.0, return_counts=True)
    assert (area.is_cuda and counts.is_cuda) if on_device else (isinstance(area, np.ndarray) and isinstance(counts, np.ndarray))
    assert host(counts).dtype == np.int32 and np.array_equal(host(counts), want)
    assert same_bits(area, areas_of(want, R, 960))
    assert same_bits(SA.sasa(x, radii=r, probe_radius=0.0), area)
    el = golden("frames_md_1JTG_uL")["q_idx"][:, 0]
    assert same_bits(SA.sasa(x, elements=el), area)         # the radius table and the default probe give the same radii
    res, c2 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, mode="residue", residue=dev(roa) if on_device else roa, return_counts=True)
    assert (res.is_cuda if on_device else isinstance(res, np.ndarray)) and np.array_equal(host(c2), want)
    assert same_bits(res, group_sums(want, R, 960, roa))
    # residue rows need not be contiguous: a permutation of the rows' names permutes the sums
    rng = np.random.default_rng(5)
    rename = rng.permutation(int(roa.max()) + 1).astype(np.int32)
    res2 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, mode="residue", residue=rename[roa])
    assert same_bits(host(res2)[:, rename], res)


def test_md_all_frames_against_frame_by_frame():
    from pesto_amd import sasa as SA
    X, R, _, want = md_case()
    area, counts = SA.shrake_rupley(X, radii=R, probe_radius=0.0, return_counts=True)
    for f in range(X.shape[0]):
        a1, c1 = SA.shrake_rupley(X[f], radii=R, probe_radius=0.0, return_counts=True)
        assert a1.shape == (X.shape[1],) and np.array_equal(c1, want[f]) and same_bits(a1, area[f])
    assert np.array_equal(counts, want)


def test_batch_in_one_launch_and_one_at_a_time():
    from pesto_amd import sasa as SA
    g = golden("sasa")
    structs = batch_structures(g)
    sizes, want, R = g["batch_sizes"].tolist(), g["batch_counts"].astype(np.int32), g["batch_R"]
    assert [s[1].shape[0] for s in structs] == sizes and any((e == "Zn").any() for _, _, e in structs)
    X = np.concatenate([s[1] for s in structs])
    area, counts = SA.shrake_rupley(X, radii=R, probe_radius=0.0, sizes=sizes, return_counts=True)
    assert np.array_equal(counts, want) and same_bits(area, areas_of(want, R, 960))
    cuts = np.cumsum(sizes)[:-1]
    for (name, xyz, el), w, a_all in zip(structs, np.split(want, cuts), np.split(area, cuts)):
        a1, c1 = SA.shrake_rupley(xyz, elements=el, return_counts=True)
        assert np.array_equal(c1, w) and same_bits(a1, a_all), name
    # the structure dicts of the reader, one and many
    dicts = [dict(xyz=xyz, element=el) for _, xyz, el in structs]
    many = SA.structure_sasa(dicts)
    assert len(many) == len(sizes) and all(same_bits(m, a) for m, a in zip(many, np.split(area, cuts)))
    assert same_bits(SA.structure_sasa(dicts[1]), many[1])
    # another order of the batch changes nothing for a structure
    back = SA.shrake_rupley(np.concatenate([s[1] for s in structs[::-1]]), radii=np.concatenate(np.split(R, cuts)[::-1]),
                            probe_radius=0.0, sizes=sizes[::-1], return_counts=True)[1]
    assert np.array_equal(np.concatenate(np.split(back, np.cumsum(sizes[::-1])[:-1])[::-1]), want)


def test_dense_candidate_lists_exceed_the_tile():
    from pesto_amd import sasa as SA
    from pesto_amd.topology import synthetic_cloud
    g = golden("sasa")
    X = synthetic_cloud(1500)
    want = g["dense_counts"].astype(np.int32)
    R = np.full(1500, 6.0, np.float32)
    area, counts = SA.shrake_rupley(X, radii=R, probe_radius=0.0, return_counts=True)
    assert np.array_equal(counts, want) and same_bits(area, areas_of(want, R, 960))
    area_d, counts_d = SA.shrake_rupley(dev(X), radii=dev(R), probe_radius=0.0, return_counts=True)
    assert np.array_equal(host(counts_d), want) and same_bits(area_d, area)


def test_every_planted_case():
    from pesto_amd import sasa as SA
    g = golden("sasa")
    for name in planted_names(g):
        X, R, P, sizes, want = planted_case(g, name)
        area, counts = SA.shrake_rupley(X, radii=R, probe_radius=0.0, n_sphere_points=P, sizes=sizes, return_counts=True)
        assert np.array_equal(counts, want), (name, counts.tolist(), want.tolist())
        with np.errstate(all="ignore"):
            assert same_bits(area, areas_of(want, R, P)), name
        area_d, counts_d = SA.shrake_rupley(dev(X), radii=dev(R), probe_radius=0.0, n_sphere_points=P, sizes=sizes, return_counts=True)
        assert np.array_equal(host(counts_d), want) and same_bits(area_d, area), name


def test_a_permutation_of_the_atoms_permutes_the_counts():
    from pesto_amd import sasa as SA
    X, R, _, want = md_case()
    perm = np.random.default_rng(9).permutation(X.shape[1])
    area, counts = SA.shrake_rupley(X[0][perm], radii=R[perm], probe_radius=0.0, return_counts=True)
    assert np.array_equal(counts, want[0][perm]) and same_bits(area, areas_of(want[0], R, 960)[perm])


def test_two_runs_give_identical_bits():
    from pesto_amd import sasa as SA
    X, R, roa, _ = md_case()
    x, r = dev(X), dev(R)
    a1, c1 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, return_counts=True)
    g1 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, mode="residue", residue=roa)
    a2, c2 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, return_counts=True)
    g2 = SA.shrake_rupley(x, radii=r, probe_radius=0.0, mode="residue", residue=roa)
    assert same_bits(a1, a2) and np.array_equal(host(c1), host(c2)) and same_bits(g1, g2)


def test_buried_area_of_a_two_chain_assembly():
    from pesto_amd import sasa as SA
    from pesto_amd.structure_io import Structure
    d = Structure.parse_pdb(gzip.open(os.path.join(GOLDEN, "pdb", "1OL5.pdb1.gz"), "rb").read()).to_dict()
    chains, sub = np.unique(d["chain_name"], return_inverse=True)
    sub = sub.reshape(-1)
    assert chains.size == 2
    X, radii = d["xyz"], SA.atomic_radii(d["element"])
    dc, da = SA.buried_area(X, radii, sub)
    assert dc.dtype == np.int32 and da.dtype == np.float32 and dc.shape == da.shape == (X.shape[0],)
    assert dc.min() >= 0 and dc.max() > 0                    # exact: the complex's occluders are a superset of the subunit's
    # atoms farther than 2 max R from the other chain lose nothing
    Rmax = float((radii + PROBE).max())
    x64 = X.astype(np.float64)
    far = np.ones(X.shape[0], bool)
    for c in (0, 1):
        mine, other = np.nonzero(sub == c)[0], x64[sub != c]
        dist = np.sqrt(((x64[mine][:, None, :] - other[None, :, :]) ** 2).sum(-1)).min(1)
        far[mine] = dist > 2.0 * Rmax
    assert far.any() and (~far).any() and not dc[far].any() and not da[far].any()
    # the same from its parts
    whole, cw = SA.shrake_rupley(X, radii=radii, return_counts=True)
    for c in (0, 1):
        alone, ca = SA.shrake_rupley(X[sub == c], radii=radii[sub == c], return_counts=True)
        assert np.array_equal(ca - cw[sub == c], dc[sub == c]) and same_bits(alone - whole[sub == c], da[sub == c])
    dcd, dad = SA.buried_area(dev(X), dev(radii), sub)
    assert dcd.is_cuda and dad.is_cuda and np.array_equal(host(dcd), dc) and same_bits(dad, da)


def test_forward_frames_then_sasa_on_the_same_device_tensor():
    import torch
    from pesto_amd import Model
    from pesto_amd import sasa as SA
    from pesto_amd.config import CONFIGS
    f = md_frames()
    _, R, roa, want = md_case()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    X = dev(f["X_frames"])
    M = torch.zeros((X.shape[1], f["R"]), device=X.device)
    M[torch.arange(X.shape[1], device=X.device), dev(f["res_of_atom"]).long()] = 1.0
    z = m.forward_frames(X, dev(f["ids"]), dev(f["q0"]), M)
    area, counts = SA.shrake_rupley(X, radii=dev(R), probe_radius=0.0, model=m, return_counts=True)
    res = SA.shrake_rupley(X, radii=dev(R), probe_radius=0.0, mode="residue", residue=roa, model=m)
    assert z.is_cuda and area.is_cuda and counts.is_cuda and res.is_cuda and tuple(res.shape) == (X.shape[0], f["R"])
    assert np.abs(host(z) - f["z"]).max() < 1e-4
    assert np.array_equal(host(counts), want) and same_bits(area, areas_of(want, R, 960)) and same_bits(res, group_sums(want, R, 960, roa))
