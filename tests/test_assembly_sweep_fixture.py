"""CPU checks of the assembly sweep (tests/assembly_sweep.py): the case lists cover every edge set; every builder keeps the sizes and
properties its construction promises; the vectorised definitions equal the restatements the suite already trusts - contacts_def against
dataset_fixture.np_contacts / np_typed_keys on every sweep case and against the recorded dataset_*.npz, chain_dist against
topology._norm_xyz, scores_def against the recorded eval_scores.npz within the bounds of test_interface_eval, patches_def's membership is
test_patches_fixture.definition by construction, labels_def against the per-pair loop."""
import numpy as np
import pytest

import assembly_sweep as S
import dataset_fixture as fx
from conftest import golden

ALL = S.all_cases()
IDS = [f"{entry}:{S.ident(case)}" for entry, case in ALL]


def test_lists_cover_the_edges():
    cov = S.coverage()
    for key, need in S.REQUIRED.items():
        assert need <= cov[key], (key, sorted(need - cov[key], key=str))
    for entry, cases in S.CASES.items():
        assert len({(f, s) for f, s, _ in cases}) == len(cases) and len({s for _, s, _ in cases}) == len(cases), entry
    n_atoms = max(S._call_sizes(shape)[0] for _, _, shape in S.CONTACTS)
    assert n_atoms <= 5120, n_atoms              # (K = 4097: two tiles of the radix sort and one key)


@pytest.mark.parametrize("entry,case", ALL, ids=IDS)
def test_case_builds_and_keeps_its_promises(entry, case):
    c = S.build(entry, case)
    family, seed, shape = case
    kind, flags = S.parse(family)
    if entry == "contacts":
        w = c["want"]
        n, n_sub, K, G = S._call_sizes(shape)
        assert c["X"].shape == (n, 3) and c["n_sub"] == n_sub and n <= 5120
        assert K is None or (w["K"], w["G"]) == (K, G), (case, w["K"], w["G"], K, G)
        assert np.all(np.diff(c["sub"]) >= 0) and c["res"].min() >= 0 and c["res"].max() < 8192 and c["typ"].min() >= -1 and c["typ"].max() < c["n_types"]
        assert w["groups"][:, 3].sum() == w["U"] == w["keys"].shape[0] == w["rkeys"].shape[0]
        if kind == "lattice":
            v = c["X"].astype(np.float64) * 16
            assert np.array_equal(v, np.round(v))
        if "untyped" in flags:
            assert w["U"] == 0 and not w["T"].any()
        if "typed" in flags:
            assert (c["typ"] >= 0).all() and w["U"] == np.unique(w["run_key"]).size
        if "mix" in flags and w["K"] > 50:
            assert 0 < w["U"] < np.unique(w["run_key"]).size
        if "r8191" in flags:
            assert c["res"].max() == 8191 and (w["keys"][:, 0] == 8191).any() and (w["keys"][:, 1] == 8191).any() and (w["keys"][:, :2] == 0).any()
        if "nt128" in flags:
            assert (w["keys"][:, 2] == 127).any() and (w["keys"][:, 3] == 127).any() and w["T"][:, 127, 127].any()
        if "planted" in flags:
            have = set(((np.repeat(np.arange(w["G"]), w["groups"][:, 3]).astype(np.int64) << 26) | (w["keys"][:, 0].astype(np.int64) << 13) | w["keys"][:, 1]).tolist())
            no, yes = c["planted"]
            assert no not in have and yes in have
            k_no, k_yes = np.nonzero(w["run_key"] == no)[0], np.nonzero(w["run_key"] == yes)[0]
            a, b = w["pairs"][:, 0], w["pairs"][:, 1]
            assert c["typ"][a[k_no[0]]] >= 0 and c["typ"][b[k_no[0]]] >= 0 and c["typ"][b[k_no[-1]]] == -1
            assert c["typ"][b[k_yes[0]]] == -1 and c["typ"][a[k_yes[-1]]] >= 0 and c["typ"][b[k_yes[-1]]] >= 0
        if any(s[0] == "fan" for s in shape):
            per_atom = np.bincount(w["pairs"][:, 0], minlength=n)
            a = int(np.argmax(per_atom))
            assert per_atom[a] >= 64
        if any(s[0] == "comb" and s[1] > 0 for s in shape):
            per_atom = np.bincount(w["pairs"][:, 0], minlength=n)
            first = int(w["pairs"][0, 0])
            assert (per_atom[first:int(w["pairs"][-1, 0])] == 0).any() or w["K"] < 8      # zero-contact atoms repeat an offset in between
    elif entry == "scores":
        sizes, C = shape
        assert c["want"].shape == (len(sizes), 8, C)
        for y, p, R, w in zip(c["ys"], c["ps"], sizes, c["want"]):
            k = p.astype(np.float64) / S.P_GRID
            assert p.dtype == np.float32 and p.shape == (R, C) and np.array_equal(k, np.round(k)) and k.min() >= 0 and k.max() <= 2 ** 24
            P = y.sum(0)
            N = R - P
            want_p = S.n_positive(family, R)
            assert want_p is None or (P == want_p).all()
            if family == "PeqN":
                assert (P == N).all()
            if family == "PgtN":
                assert (P > N).all()
            if family in ("distinct", "P1", "N1", "PeqN", "PgtN", "allpos", "allneg"):
                assert all(np.unique(p[:, c_]).size == R for c_ in range(C))
            if family == "grid8":
                assert all(np.unique(p[:, c_]).size <= 8 for c_ in range(C))
            if family == "half":
                assert set(np.unique(p).tolist()) <= {0.5, float(np.nextafter(np.float32(0.5), np.float32(1)))}
            if family == "const":
                assert all(np.unique(p[:, c_]).size == 1 for c_ in range(C))
            assert np.array_equal(np.isnan(w[6]), (P == 0) | (N == 0)) and np.isnan(w[7]).all() == (R == 1)
    elif entry == "patches":
        structs, C = shape
        R = sum(p.shape[0] for p in c["ps"])
        assert R <= 4097 + 4096 + 64 and c["patch_of"].shape == (len(c["sels"]), R) and len(c["sels"]) == C * (C + 1) // 2
        o = 0
        for s, ((graph, n, layout), p, nodes) in enumerate(zip(structs, c["ps"], c["nodes"])):
            lab = c["patch_of"][:, o:o + p.shape[0]]
            assert p.shape[0] <= 4097
            if "varied" not in flags:
                assert nodes.size == n and all(np.array_equal(np.nonzero(l >= 0)[0], nodes) for l in lab), (case, s)
                npch = c["n_patches"][s]
                assert (npch == npch[0]).all()
                if graph == "dust":
                    assert npch[0] == n
                if graph in ("star", "clique", "twocliques") and n:
                    assert npch[0] == 1
                if graph == "chain" and n:
                    assert 1 <= npch[0] <= (n // 10 if n >= 100 else n)        # (a 12 A gap at about one step in fifty)
                if graph == "lattice":
                    x = c["xyzs"][s][nodes[:6]].astype(np.float32)
                    d = x[1::2] - x[0::2]
                    ss = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
                    assert ss.dtype == np.float32 and ss[0] == 100 and ss[1] == np.nextafter(np.float32(100), np.float32(0)) and ss[2] < ss[1]
                    assert np.sqrt(ss[0]) == 10 and np.sqrt(ss[1]) == 10 and np.sqrt(ss[2]) < 10
                    l0 = lab[0][nodes[:6]]
                    assert l0[0] != l0[1] and l0[2] != l0[3] and l0[4] == l0[5]
                if graph == "twocliques":
                    x = c["xyzs"][s][nodes].astype(np.float32)
                    D = np.sqrt(np.sum(np.square(x[None, :256] - x[256:, None]), axis=2))
                    assert np.argwhere(D < 10).tolist() == [[0, 255]]              # the one edge: node 256 with node 255
            o += p.shape[0]
        assert (c["patch_size"].sum(1) == (c["patch_of"] >= 0).sum(1)).all()
    else:
        assert c["labels"].any() and not c["labels"].all() and (c["mask"] == 0).any() and (c["mask"] == np.uint32(1 << 31)).any()
        assert 0 < c["receptor"].sum() < c["receptor"].size and np.bincount(c["res"]).max() >= 2
        if kind == "lattice":
            assert c["ties"].any()


# ------------------------------------------------------------------ contacts_def is np_contacts / np_typed_keys, chain_dist is _norm_xyz
def _as_subunits(c, s):
    """assembly s of a contacts case as the reference's {name: {xyz, resid, resname}} with molecule ids T0 .. T<nt-1>"""
    return {name: {"xyz": xyz, "resid": res, "resname": np.array([f"T{t}" if t >= 0 else "none" for t in typ])} for name, xyz, res, typ, _ in c["rows"][s]}


@pytest.mark.parametrize("case", S.CONTACTS, ids=S.ident)
def test_contacts_def_is_the_reference_restatement(case):
    from pesto_amd.topology import _norm_xyz
    c = S.build("contacts", case)
    w = c["want"]
    mids = [f"T{t}" for t in range(c["n_types"])]
    g = 0
    for s in range(len(c["rows"])):
        subs = _as_subunits(c, s)
        o0, o1 = int(c["offs"][s]), int(c["offs"][s + 1])
        x = c["X"][o0:o1]
        for c0 in range(0, o1 - o0, 512):
            assert np.array_equal(S.chain_dist(x[c0:c0 + 512], x).astype(np.float32), _norm_xyz(x[c0:c0 + 512, None, :] - x[None, :, :]).astype(np.float32)), case
        start = {name: o0 + int(np.nonzero(c["sub"][o0:o1] == c["sub"][o0] + k)[0][0]) for k, name in enumerate(subs)}
        for ci, cj, ids, d in fx.np_contacts(subs):
            p0 = int(w["groups"][g, 2])
            p1 = int(w["groups"][g + 1, 2]) if g + 1 < w["G"] else w["K"]
            assert np.array_equal(w["pairs"][p0:p1].astype(np.int64) - [start[ci], start[cj]], ids), (case, ci, cj)
            assert w["d"][p0:p1].tobytes() == d.astype(np.float32).tobytes(), (case, ci, cj)
            Y, T = fx.np_typed_keys(subs[ci], subs[cj], ids, mids)
            u0, u1 = (np.unique(subs[k]["resid"]) for k in (ci, cj))
            Y = np.stack([u0[Y[:, 0]], u1[Y[:, 1]], Y[:, 2], Y[:, 3]], 1).astype(np.uint16).reshape(-1, 4)      # dense residue columns -> the case's
            k0 = int(w["groups"][:g, 3].sum())
            k1 = k0 + int(w["groups"][g, 3])
            assert np.array_equal(w["keys"][k0:k1], Y), (case, ci, cj)
            assert np.array_equal(w["rkeys"][k0:k1], np.unique(Y[:, [1, 0, 3, 2]], axis=0).reshape(-1, 4)), (case, ci, cj)
            assert np.array_equal(w["T"][g].astype(bool), T), (case, ci, cj)
            g += 1
    assert g == w["G"]


@pytest.mark.parametrize("name", [n for n in fx.CASES if n != "monomer"])
def test_contacts_def_is_the_recorded_dataset(name):
    from pesto_amd import dataset
    g = fx.load(name)
    g = {k: g[k] for k in g.files}                      # (every array read once: the readers index the archive again and again)
    rows = dataset._subunit_rows(fx.subunits_of(name), dataset.MOLECULE_IDS)
    X, res, typ = (np.concatenate([r[k] for r in rows]) for k in (1, 2, 3))
    sub = np.repeat(np.arange(len(rows)), [r[1].shape[0] for r in rows]).astype(np.int32)
    start = dict(zip([r[0] for r in rows], np.cumsum([0] + [r[1].shape[0] for r in rows])))
    w = S.contacts_def(X, sub, res, typ, np.array([0, X.shape[0]]), len(dataset.MOLECULE_IDS))
    ref = {(ci, cj): (ids, d) for ci, cj, ids, d in fx.contacts(g)}
    assert len(ref) == 2 * w["G"]
    ds, at = fx.unpack(g, "ds"), fx.attrs(g)
    key = f"{str(g['pdbid']).upper()[1:3]}/{str(g['pdbid']).upper()}/{g['bid']}"
    names = [r[0] for r in rows]
    for x in range(w["G"]):
        ci, cj = names[w["groups"][x, 0]], names[w["groups"][x, 1]]
        p0, p1 = int(w["groups"][x, 2]), int(w["groups"][x + 1, 2]) if x + 1 < w["G"] else w["K"]
        ids, d = ref[(ci, cj)]
        assert np.array_equal(w["pairs"][p0:p1].astype(np.int64) - [start[ci], start[cj]], ids) and w["d"][p0:p1].tobytes() == d.tobytes(), (name, ci, cj)
        assert np.array_equal(ref[(cj, ci)][0], ids[:, ::-1])
        k0 = int(w["groups"][:x, 3].sum())
        k1 = k0 + int(w["groups"][x, 3])
        for a, b, rows_k, T in ((ci, cj, w["keys"][k0:k1], w["T"][x]), (cj, ci, w["rkeys"][k0:k1], w["T"][x].T)):
            p = f"data/contacts/{key}/{a}/{b}"
            if k1 == k0:
                assert p + "/Y" not in ds, p
                continue
            assert np.array_equal(rows_k, ds[p + "/Y"]) and np.array_equal(T.astype(bool), at[p]["ctype"]), p


# ------------------------------------------------------------------ scores_def against the recorded reference
def test_scores_def_reproduces_the_recorded_scores():
    s = golden("eval_scores")
    equal = total = 0
    for case in s["cases"].astype(str):
        y, p, off, ref = (s[f"{case}_{k}"] for k in ("y", "p", "offsets", "scores"))
        got = np.stack([S.scores_def(y[off[i]:off[i + 1]], p[off[i]:off[i + 1]]) for i in range(off.size - 1)])
        ref = np.asarray(ref, np.float32)
        assert got.shape == ref.shape and np.array_equal(np.isnan(got), np.isnan(ref)), case
        ok = ~np.isnan(ref)
        tol = np.full(ref.shape, 1e-6, np.float32)
        tol[..., 5, :] = 1e-5
        err = np.abs(got - ref)
        assert np.all(err[ok] <= tol[ok]), (case, float(err[ok].max()))
        equal += int((got[ok].view(np.int32) == ref[ok].view(np.int32)).sum())
        total += int(ok.sum())
    print(f"scores_def against eval_scores.npz: {equal} of {total} finite entries bit-equal")
    assert total > 0


def test_scores_def_counts_pairs_as_the_pair_loop():
    """the sorted count of 2 (p+ > p-) + (p+ == p-) against every pair, on a tie-heavy case"""
    c = S.build("scores", S.SCORES[1])
    for y, p, w in zip(c["ys"], c["ps"], c["want"]):
        for k in range(p.shape[1]):
            pp, pn = p[y[:, k] != 0, k], p[y[:, k] == 0, k]
            if pp.size and pn.size:
                u2 = 2 * int((pp[:, None] > pn[None, :]).sum()) + int((pp[:, None] == pn[None, :]).sum())
                assert w[6, k] == np.float32(u2 / (2.0 * pp.size * pn.size))


# ------------------------------------------------------------------ labels_def against the per-pair loop
@pytest.mark.parametrize("case", S.LABELS, ids=S.ident)
def test_labels_def_is_the_brute_force(case):
    from pesto_amd.topology import _norm_xyz
    c = S.build("labels", case)
    labels = np.zeros(c["n_res"], np.uint32)
    for s in range(len(c["sizes"])):
        o0, o1 = int(c["offs"][s]), int(c["offs"][s + 1])
        D = _norm_xyz(c["X"][o0:o1, None, :] - c["X"][None, o0:o1, :]).astype(np.float32)
        for a in range(o0, o1):
            if c["receptor"][a]:
                for b in range(o0, o1):
                    if c["sub"][a] != c["sub"][b] and D[a - o0, b - o0] < np.float32(S.R_THR):
                        labels[c["res"][a]] |= c["mask"][b]
    assert np.array_equal(labels, c["labels"])
