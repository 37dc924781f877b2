"""GPU tests of pesto_amd.evaluate: interface labels (pesto_interface_labels) against the reference's labels of the 16 assemblies of
tests/golden/eval_labels.npz, bc_scoring (pesto_bc_scores) against the reference's bc_scoring (eval_scores.npz), and the
benchmark_assemblies driver on three assemblies."""
import gzip
import os
import shutil

import numpy as np
import pytest

from conftest import GOLDEN, golden, weights

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def model():
    import torch
    from pesto_amd import Model
    from pesto_amd.config import CONFIGS
    assert torch.cuda.is_available()
    m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
    m.load_state_dict(weights("i_v4_0"))
    return m


def _assemblies():
    """[(name, {subunit: {xyz, resname, resid}}, {subunit: reference labels})] of the fixture."""
    g = golden("eval_labels")
    table = g["resname_table"].astype(str)
    names, out = g["names"].astype(str), []
    for a, name in enumerate(names):
        subs, ref = {}, {}
        for k in np.where(g["sub_assembly"] == a)[0]:
            me = g["atom_sub"] == k
            sn = g["sub_names"][k].decode()
            subs[sn] = {"xyz": g["X"][me], "resname": table[g["atom_resname"][me]], "resid": g["atom_res"][me]}
            ref[sn] = g["labels"][g["res_offsets"][k]:g["res_offsets"][k + 1]]
        out.append((name, subs, ref))
    return out


def _compare(got, ties, ref):
    """number of residues that disagree (asserted to be tie-flagged)"""
    n = 0
    for sn, y in ref.items():
        bad = np.any(got[sn] != y, axis=1)
        assert not np.any(bad & ~ties[sn]), (sn, np.where(bad & ~ties[sn])[0])
        n += int(bad.sum())
    return n


def test_labels_match_reference_all16_one_launch(model):
    from pesto_amd.evaluate import interface_labels_batch
    asm = _assemblies()
    got, ties = interface_labels_batch(model, [a[1] for a in asm], return_ties=True)
    n_bad = n_tie = 0
    for (name, _, ref), gl, tl in zip(asm, got, ties):
        assert list(gl) == list(ref), name
        n_bad += _compare(gl, tl, ref)
        n_tie += sum(int(t.sum()) for t in tl.values())
    print(f"16 assemblies: {sum(len(a[2]) for a in asm)} subunits, {n_bad} residue(s) differ (all on fp32 ties), {n_tie} tie-flagged residues")
    assert n_bad == 0 or n_bad <= n_tie


def test_labels_batch_single_host_device_identical(model):
    from pesto_amd.evaluate import interface_labels, interface_labels_batch
    asm = _assemblies()
    batch = interface_labels_batch(model, [a[1] for a in asm])
    dev = interface_labels_batch(model, [a[1] for a in asm], on_device=True)
    for (name, subs, _), b, d in zip(asm, batch, dev):
        one = interface_labels(model, subs)
        for sn in subs:
            assert np.array_equal(one[sn], b[sn]) and np.array_equal(d[sn], b[sn]), (name, sn)


def test_labels_classes_and_threshold(model):
    """32 single-residue classes (config.py:22's alternative r_types) and a different threshold against a brute-force host pass."""
    import torch
    from pesto_amd.evaluate import CATEG_TO_RESNAMES, interface_labels, resname_masks
    name, subs, _ = [a for a in _assemblies() if a[0] == "1ZNS"][0]
    r_types = [[c] for c in CATEG_TO_RESNAMES["protein"]] + [[c] for c in CATEG_TO_RESNAMES["ion"][:12]]
    assert len(r_types) == 32
    got = interface_labels(model, subs, r_thr=4.0, r_types=r_types)
    for sn, s in subs.items():
        rec, _ = resname_masks(s["resname"], r_types=r_types)
        y = np.zeros((int(s["resid"].max()) + 1, 32), bool)
        for on, o in subs.items():
            if on == sn:
                continue
            _, mask = resname_masks(o["resname"], r_types=r_types)
            D = torch.norm(torch.from_numpy(s["xyz"]).unsqueeze(1) - torch.from_numpy(o["xyz"]).unsqueeze(0), dim=2).numpy()
            ia, ib = np.where(D < 4.0)
            for i, j in zip(ia, ib):
                if rec[i]:
                    y[s["resid"][i]] |= ((int(mask[j]) >> np.arange(32)) & 1).astype(bool)
        assert np.array_equal(got[sn], y), sn


def _golden_cases():
    s = golden("eval_scores")
    return {c: {k: s[f"{c}_{k}"] for k in ("y", "p", "offsets", "scores")} for c in s["cases"].astype(str)}


def _check_scores(got, ref, tag):
    got, ref = np.asarray(got, np.float32), np.asarray(ref, np.float32)
    assert got.shape == ref.shape, tag
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (tag, np.argwhere(np.isnan(got) != np.isnan(ref))[:5])
    ok = ~np.isnan(ref)
    tol = np.full(ref.shape, 1e-6, np.float32)
    tol[..., 5, :] = 1e-5                                  # mcc
    err = np.abs(got - ref)
    assert np.all(err[ok] <= tol[ok]), (tag, float(err[ok].max()))


@pytest.mark.parametrize("case", ["pdbs53_logits", "pdbs53_bfactor", "synth"])
@pytest.mark.parametrize("where", ["host", "device"])
def test_bc_scores_match_reference(model, case, where):
    import torch
    from pesto_amd.evaluate import bc_scores_batch, bc_scoring
    d = _golden_cases()[case]
    off = d["offsets"]
    ys = [d["y"][off[i]:off[i + 1]] for i in range(off.size - 1)]
    ps = [d["p"][off[i]:off[i + 1]] for i in range(off.size - 1)]
    if where == "device":
        ys = [torch.from_numpy(y).cuda() for y in ys]
        ps = [torch.from_numpy(p).cuda() for p in ps]
    got = bc_scores_batch(model, ys, ps)
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    if where == "device":                                 # the same call from host memory (CPU tensors): the same bits
        host = bc_scores_batch(model, [y.cpu() for y in ys], [p.cpu() for p in ps])
        assert isinstance(host, torch.Tensor) and np.array_equal(got, host.numpy(), equal_nan=True)
    _check_scores(got, d["scores"], f"{case}/{where}")
    for i in (0, off.size - 2):                           # the single-structure form (its own weightless handle)
        one = bc_scoring(ys[i], ps[i])
        _check_scores(one.cpu().numpy() if hasattr(one, "cpu") else one, d["scores"][i], f"{case}/{where}/{i}")


def _np_scores(y, p):
    """bc_scoring restated in numpy (float64) from y [R, C], p [R, C]"""
    y = y.astype(bool)
    q = np.rint(p.astype(np.float64)) != 0
    TP, FP = (y & q).sum(0).astype(np.float64), (~y & q).sum(0).astype(np.float64)
    P = y.sum(0).astype(np.float64)
    N = y.shape[0] - P
    FN, TN = P - TP, N - FP
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = (TP + TN) / (TP + TN + FP + FN)
        ppv = np.where(P > 0, TP / (TP + FP), np.nan)
        npv = np.where(N > 0, TN / (TN + FN), np.nan)
        fin = lambda v: np.where(np.isinf(v), np.nan, v)
        tpr, tnr = fin(TP / (TP + FN)), fin(TN / (TN + FP))
        mcc = fin((TP * TN - FP * FN) / np.sqrt((TP + FP) * (TP + FN) * (TN + FP) * (TN + FN)))
    auc = np.full(y.shape[1], np.nan)
    for c in range(y.shape[1]):
        pp, pn = p[y[:, c], c], p[~y[:, c], c]
        if pp.size and pn.size:
            auc[c] = ((pp[:, None] > pn[None, :]).sum() + 0.5 * (pp[:, None] == pn[None, :]).sum()) / (pp.size * pn.size)
    std = np.std(p.astype(np.float64), axis=0, ddof=1)
    return np.stack([acc, ppv, npv, tpr, tnr, mcc, auc, std])


def test_benchmark_assemblies(model, tmp_path):
    from pesto_amd.evaluate import BC_SCORE_NAMES, benchmark_assemblies
    ref = {a[0]: a[2] for a in _assemblies()}
    paths = []
    for name in ("1ZNS", "1H9D", "1OL5"):          # DNA + ions, DNA, ions + ligands
        p = tmp_path / f"{name}.pdb1"
        with gzip.open(os.path.join(GOLDEN, "pdb", name + ".pdb1.gz"), "rb") as fi, open(p, "wb") as fo:
            shutil.copyfileobj(fi, fo)
        paths.append(str(p))
    errors = []
    records, summary = benchmark_assemblies(model, paths + [str(tmp_path / "missing.pdb1")], on_error=errors.append)
    assert len(errors) == 1
    want = [(n, sn) for n in ("1ZNS", "1H9D", "1OL5") for sn, y in ref[n].items() if y.any()]
    got = [(os.path.basename(r["file"])[:-5], r["subunit"]) for r in records]
    assert got == want
    for r in records:
        y = ref[os.path.basename(r["file"])[:-5]][r["subunit"]]
        assert np.array_equal(r["y"], y) and r["residues"] == y.shape[0] and r["p"].shape == y.shape
        exp = _np_scores(r["y"], r["p"])
        assert np.array_equal(np.isnan(r["scores"]), np.isnan(exp)), r["subunit"]
        ok = ~np.isnan(exp)
        assert np.all(np.abs(r["scores"][ok] - exp[ok]) <= 1e-5), r["subunit"]
    assert list(summary) == BC_SCORE_NAMES
    allsc = np.stack([r["scores"] for r in records])
    for i, k in enumerate(BC_SCORE_NAMES):
        for c in range(5):
            col = allsc[:, i, c]
            col = col[~np.isnan(col)]
            assert (np.isnan(summary[k][c]) and col.size == 0) or np.isclose(summary[k][c], np.median(col))
    kept = benchmark_assemblies(model, paths, min_num_res=200)[0]
    assert [(r["file"], r["subunit"]) for r in kept] == [(r["file"], r["subunit"]) for r in records if r["residues"] >= 200]
