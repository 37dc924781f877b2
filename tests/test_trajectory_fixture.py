"""CPU checks of the MD-analysis fixture (tests/golden/make_trajectory_golden.py) and of the host side of pesto_amd.trajectory: the
reference's recorded outputs equal a NumPy restatement of the definitions (counts, P, maps, native contacts and fnat exactly; L, KL, the
superposition, rmsd and the centroids against float64 within the reference's recorded deviation), the planted distances land where the
definition says, and bad arguments raise ValueError before any launch. For the two large outputs, superposed coordinates and centroids,
the fixture records the reference's deviation and a sub-sample of its output only (file size): their float64 yardstick is this file's own
restatement (superpose64 from the recorded-and-checked t, R, t_ref; centroids64), in the GPU tests too."""
import numpy as np
import pytest

from conftest import golden

EPS32 = float(np.finfo(np.float32).eps)
BINS = np.linspace(0.0, 10.0, 21)
CONTACT_CASES = ["iface", "iface_other", "planted_b64", "planted_b1", "planted_self"]


def from256(q, nm=False):
    """the fixture's coordinates: multiples of 1/256 A; nm: float32(A) * float32(0.1)"""
    x = (q.astype(np.float64) / 256.0).astype(np.float32)
    return x * np.float32(0.1) if nm else x


def contact_inputs(g, case):
    """(xyz0, xyz1 or None for a trajectory against itself, bins)"""
    if case.startswith("planted"):
        return (g["planted_b"], None, g[case + "_bins"]) if case == "planted_self" else (g["planted_a"], g["planted_b"], g[case + "_bins"])
    return from256(g[case + "_a256"]), from256(g[case + "_b256"]), g[case + "_bins"]


def dist(x0, x1):
    """float32 [F, Na, Nb]: sqrt((dx*dx + dy*dy) + dz*dz), NumPy's correctly rounded float32 operations"""
    return np.sqrt(np.sum(np.square(x0[:, :, None, :] - x1[:, None, :, :]), -1))


def hits(x0, x1, bins):
    """int [F, Na, Nb]: the b with bins[b] <= d < bins[b+1] in float64, -1 for none"""
    d = dist(x0, x1).astype(np.float64)
    b = np.searchsorted(bins, d, side="right") - 1
    return np.where((d >= bins[0]) & (d < bins[-1]), b, -1)


def counts_def(x0, x1, bins):
    h = hits(x0, x0 if x1 is None else x1, bins)
    c = np.zeros(h.shape[1:] + (len(bins) - 1,), np.int64)
    for b in range(len(bins) - 1):
        c[..., b] = (h == b).sum(0)
    return c


def p_of_counts(c):
    return c.astype(np.float32) / (c.sum(-1).astype(np.float32) + np.float32(1e-6))[..., None]


def loglik64(x0, x1, bins, P):
    h = hits(x0, x1, bins)
    p = np.take_along_axis(P.astype(np.float64)[None], np.maximum(h, 0)[..., None], -1)[..., 0]
    return -np.where(h >= 0, np.log(1.0 - p + np.floor(p)), 0.0).sum((1, 2)) / P.size


def kl64(P, Q):
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    R = Q / (P + np.float64(np.float32(1e-6)))
    R[R < np.float64(np.float32(1e-6))] = 1.0
    return -np.sum(P * np.log(R), -1)


def superpose64(ref, xyz):
    """(t, R, t_ref) in float64 from the float32 inputs"""
    ref, xyz = ref.astype(np.float64), xyz.astype(np.float64)
    t, tr = xyz.mean(1, keepdims=True), ref.mean(1, keepdims=True)
    U, _, Vt = np.linalg.svd(np.einsum("fna,fnb->fab", ref - tr, xyz - t))
    Vt[:, 2] *= np.sign(np.linalg.det(U) * np.linalg.det(Vt))[:, None]                   # the reflection folded into the last right vector
    return t, np.einsum("fka,fbk->fab", Vt, U), tr


def maps_def(xa, xb, res_a, res_b, r_thr, scale=10.0):
    c = dist(xa, xb) * np.float32(scale) < np.float32(r_thr)
    m = np.zeros((xa.shape[0], int(res_a.max()) + 1, int(res_b.max()) + 1), np.uint8)
    for r in range(m.shape[1]):
        rows = c[:, res_a == r].any(1)
        for s in range(m.shape[2]):
            m[:, r, s] = rows[:, res_b == s].any(1)
    return m


def superpose_inputs(g, tag):
    """(xyz_ref, xyz, selection or None) of a superposition case; the frames are those of frames_md_1JTG_uL.npz"""
    X = golden("frames_md_1JTG_uL")["X_frames"]
    if tag == "mirror":
        return X[:1], X[5:6] * np.array([1, 1, -1], np.float32), None
    return X[:1], X, (g["superpose_sel"].astype(np.int64) if tag == "sel" else None)


def tolerance(g, key, value64):
    """the issue's bound for a floating-point output: max(4 e_ref, 4 eps32 max|value|) around the float64 values"""
    return max(4.0 * float(g[key + "_eref"]), 4.0 * EPS32 * float(np.max(np.abs(value64))))


@pytest.mark.parametrize("case", CONTACT_CASES)
def test_counts_are_the_definition(case):
    g = golden("trajectory")
    x0, x1, bins = contact_inputs(g, case)
    assert np.array_equal(g[case + "_counts"], counts_def(x0, x1, bins))


def test_iface_covers_the_bins():
    g = golden("trajectory")
    c = g["iface_counts"]
    assert c.shape == (274, 285, 20) and g["iface_a256"].shape[0] == 64 and np.array_equal(g["iface_bins"], BINS)
    hit = c.sum(-1) > 0
    assert hit.mean() >= 0.1 and ((c > 0).sum(-1) >= 2).sum() >= 0.5 * hit.sum()
    assert g["iface10_a256"].shape == (32, 707, 3) and g["iface10_b256"].shape == (32, 701, 3)
    assert g["iface10_res_a"].max() == 90 and g["iface10_res_b"].max() == 86


def test_planted_distances_land_where_the_definition_says():
    g = golden("trajectory")
    t = g["planted_targets"]
    n = t.size
    assert np.isnan(t).sum() == 1 and (t == 0).sum() == 1 and (t == 100).sum() == 1
    # every planted point lies at exactly its target from the origin
    d = dist(g["planted_a"][:, :1], g["planted_b"])[:, 0]
    for f in range(3):
        assert np.array_equal(d[f], np.roll(t, f), equal_nan=True)
    for case in ("planted_b64", "planted_b1"):
        bins = g[case + "_bins"]
        want = np.zeros((n, bins.size - 1), np.int64)
        for j in range(n):
            for f in range(3):
                v = float(t[(j - f) % n])                               # float32 target against the float64 edges, scalar by scalar
                for b in range(bins.size - 1):
                    if bins[b] <= v < bins[b + 1]:
                        want[j, b] += 1
        assert np.array_equal(g[case + "_counts"][0], want)
        assert not g[case + "_counts"][1].any() and not g[case + "_counts"][2].any()      # the NaN atom and the far one
    bins = g["planted_b64_bins"]
    assert bins.size == 65 and np.any(bins.astype(np.float32).astype(np.float64) != bins) and g["planted_b1_bins"].size == 2
    for k in (3, 7, 30):                                                # edges that are not float32 values: below | at-or-above
        lo, at, hi = (float(v) for v in t[[i for i in range(n) if abs(float(t[i]) - bins[k]) < 1e-6]])
        assert lo < bins[k] <= at < hi
    # the contact-map threshold: d * 10 < 5 fails at exactly 0.5, holds one ulp below
    mt = g["plantedmap_targets"]
    m = g["plantedmap_t5_maps"]
    assert mt[1] == np.float32(0.5) and m[0, 0, 0] == 1 and m[0, 0, 1] == 0 and m[0, 0, 2] == 0
    assert m[0, 0, 6] == 1 and not m[:, 1].any()                       # the pair at distance 0; the far single-atom residue
    assert np.bincount(g["plantedmap_res_a"]).min() == 1


def test_floating_point_outputs_against_float64():
    g = golden("trajectory")
    xa, xb, bins = contact_inputs(g, "iface")
    ya, yb, _ = contact_inputs(g, "iface_other")
    P, Q = p_of_counts(g["iface_counts"]), p_of_counts(g["iface_other_counts"])
    L0, L = loglik64(xa, xb, bins, P), loglik64(ya, yb, bins, P)
    for key, v in (("iface_L0", L0), ("iface_L", L), ("iface_Lrel", L / L0.mean()), ("iface_KL", kl64(Q, P))):
        assert np.allclose(g[key + "_f64"], v, rtol=1e-12, atol=1e-15), key
        assert np.abs(g[key + "_ref"].astype(np.float64) - v).max() <= float(g[key + "_eref"]) * (1 + 1e-12), key
    assert L0.min() > 0 and g["iface_KL_f64"].max() > 1.0


@pytest.mark.parametrize("tag", ["all", "sel", "mirror"])
def test_superposition_against_float64(tag):
    g = golden("trajectory")
    ref, xyz, sel = superpose_inputs(g, tag)
    yr, xr = (ref, xyz) if sel is None else (ref[:, sel], xyz[:, sel])
    t, R, tr = superpose64(yr, xr)
    sup = (xyz.astype(np.float64) - t) @ R + tr
    rm = np.sqrt(np.mean(np.sum(np.square((sup if sel is None else sup[:, sel]) - yr.astype(np.float64)), axis=2), axis=1)) * 10.0
    for key, v in (("t", t), ("R", R), ("tref", tr), ("rmsd", rm)):
        key = f"superpose_{tag}_{key}"
        assert np.allclose(g[key + "_f64"], v, rtol=1e-9, atol=1e-11), key
        assert np.abs(g[key + "_ref"].astype(np.float64) - v).max() <= float(g[key + "_eref"]) * (1 + 1e-6) + 1e-12, key
    key = f"superpose_{tag}_xyz"
    assert np.abs(g[key + "_ref"].astype(np.float64) - sup[:, ::32]).max() <= float(g[key + "_eref"]) * (1 + 1e-6)
    assert np.allclose(np.linalg.det(R), 1.0)
    if tag == "mirror":
        assert rm[0] > 1.0


def test_maps_and_centroids():
    g = golden("trajectory")
    xa, xb = from256(g["iface10_a256"], True), from256(g["iface10_b256"], True)
    for tag, r_thr in (("t5", 5.0), ("t41", 4.1)):
        m = maps_def(xa, xb, g["iface10_res_a"], g["iface10_res_b"], r_thr)
        assert np.array_equal(g[f"iface10_{tag}_maps"], m)
        nat = (m & m[:1]).sum((1, 2))
        assert np.array_equal(g[f"iface10_{tag}_native"], nat) and np.array_equal(g[f"iface10_{tag}_fnat"], nat / m[:1].sum())
        assert np.unique(g[f"iface10_{tag}_fnat"]).size >= 8
        pm = maps_def(g["plantedmap_a"], g["plantedmap_b"], g["plantedmap_res_a"], g["plantedmap_res_b"], r_thr)
        assert np.array_equal(g[f"plantedmap_{tag}_maps"], pm)
    f = golden("frames_md_1JTG_uL")
    c64 = centroids64(f["X_frames"], f["res_of_atom"])
    assert np.abs(g["centroids_ref"].astype(np.float64) - c64).max() <= float(g["centroids_eref"]) * (1 + 1e-9)


def centroids64(X, roa):
    R = int(roa.max()) + 1
    out = np.zeros((X.shape[0], R, 3))
    np.add.at(out, (slice(None), roa.astype(np.int64)), X.astype(np.float64))
    return out / np.bincount(roa, minlength=R)[None, :, None]


def test_arguments_raise_before_any_launch():
    from pesto_amd import trajectory as T
    m = object()                # no handle: the checks must come first
    x, y = np.zeros((4, 5, 3), np.float32), np.zeros((4, 6, 3), np.float32)
    for bad in ([0.0, 1.0, 1.0], [0.0, 2.0, 1.0], [0.0, np.nan], [0.0, np.inf], [0.0], [0.0, 1e39], np.arange(T.MAX_BINS + 2.0)):
        with pytest.raises(ValueError, match="bins"):
            T.contacts_distribution(x, y, bad, model=m)
        with pytest.raises(ValueError, match="bins"):
            T.contact_counts(x, bins=bad, model=m)
    with pytest.raises(ValueError, match="bins"):
        T.StatisticalContactsModel(0.0, 10.0, T.MAX_BINS + 2, model=m)
    with pytest.raises(ValueError, match="bins"):
        T.StatisticalContactsModel(1.0, 1.0, 5, model=m)
    assert T.MAX_BINS >= 64
    with pytest.raises(ValueError, match="frames"):
        T.contacts_distribution(x, y[:3], BINS, model=m)
    with pytest.raises(ValueError):
        T.contacts_distribution(x[0], y, BINS, model=m)
    with pytest.raises(ValueError):
        T.contacts_distribution(x[:, :, :2], y, BINS, model=m)

    class Traj:
        def __init__(self, xyz):
            self.xyz = xyz
    # shapes alone decide these: the views below repeat one element
    big = Traj(np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (2 ** 24 + 1, 1, 3), (0, 0, 0)))
    with pytest.raises(ValueError, match="2\\*\\*24"):
        T.contact_counts(big, bins=BINS, model=m)
    wide = np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (1, 20000, 3), (0, 0, 0))
    with pytest.raises(ValueError, match="too large"):
        T.contact_counts(wide, bins=BINS, model=m)
    scm = T.StatisticalContactsModel(0.0, 10.0, 21, model=m)
    assert np.array_equal(scm.bins, BINS)
    with pytest.raises(ValueError, match="fit"):
        scm.loglikelihood(x, y)
    scm.P = np.zeros((5, 6, 19), np.float32)
    with pytest.raises(ValueError, match="P must be"):
        scm.loglikelihood(Traj(x), Traj(y))
    with pytest.raises(ValueError):
        T.div_KL(np.zeros((5, 6, 20), np.float32), np.zeros((5, 6, 19), np.float32), model=m)
    ra, rb = np.array([0, 0, 1, 1, 2]), np.array([0, 1, 2, 3, 4, 5])
    for kw in (dict(res_a=ra[:4]), dict(res_b=np.array([0, 1, 2, 3, 5, 5])), dict(res_a=-ra), dict(r_thr=np.nan), dict(scale=0.0), dict(scale=np.inf),
               dict(res_a=ra.astype(np.float32)), dict(xyz_b=y[:2])):
        args = dict(xyz_a=x, xyz_b=y, res_a=ra, res_b=rb, model=m)
        args.update(kw)
        with pytest.raises(ValueError):
            T.residue_contact_maps(**args)
    with pytest.raises(ValueError, match="atoms"):
        T.residue_contact_maps(np.zeros((1, T.MAX_MAP_ATOMS, 3), np.float32), y[:1], np.zeros(T.MAX_MAP_ATOMS, int), rb, model=m)
    maps = np.zeros((4, 3, 6), np.uint8)
    for ref in (maps[:2], maps[:, :2], maps[0]):
        with pytest.raises(ValueError):
            T.fnat(ref, maps, model=m)
        with pytest.raises(ValueError):
            T.native_contacts(ref, maps, model=m)
    with pytest.raises(ValueError, match="at least 3"):
        T.superpose(x[:1], x, sel_ref=[0, 1], sel=[0, 1], model=m)
    with pytest.raises(ValueError, match="length"):
        T.rmsd(x[:1], x, sel_ref=[0, 1, 2], sel=[0, 1, 2, 3], model=m)
    with pytest.raises(ValueError):
        T.superpose(x[:1], x, sel_ref=[0, 1, 2], sel=[0, 1, 5], model=m)
    with pytest.raises(ValueError):
        T.superpose(x[:2], x, model=m)
    with pytest.raises(ValueError):
        T.superpose_transform(y[:1], x, model=m)
    with pytest.raises(ValueError):
        T.superpose_transform(x[:1, :2], x[:, :2], model=m)
    with pytest.raises(ValueError):
        T.residue_centroids(x, np.array([0, 0, 1, 1, 3]), 3, model=m)
    with pytest.raises(ValueError):
        T.residue_centroids(x, np.array([0, 0, 1, 1]), 3, model=m)
