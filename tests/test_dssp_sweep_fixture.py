"""CPU checks of the DSSP sweep's generators (tests/dssp_sweep.py) and of the definition they rest on: dssp() of
tests/golden/make_dssp_golden.py regenerates every stored array of dssp.npz exactly, with the detail dict and without; every case builds
twice to identical bytes within its attempts, flags no near-threshold decision, has the properties it promises (read from the definition's
bridges, ladders and component roots) and the structural invariants of the golden; the case list covers every edge set."""
import re
import time

import numpy as np
import pytest

import dssp_sweep as S
from conftest import golden
from test_dssp_fixture import BLANK, B, E, G, H, I, NA, S as BEND, T, case as golden_case, planted_names

IDS = [S.case_id(c) for c in S.CASES]


def test_definition_regenerates_the_golden_with_and_without_detail():
    g = golden("dssp")
    t0 = time.perf_counter()
    for name in ["batch", "frames"] + ["planted_" + n for n in planted_names(g)]:
        X, (table, pro, chain), sizes, codes, partners, em = golden_case(g, name)
        for f in range(X.shape[0]):
            r0 = 0
            for n in sizes:
                args = (X[f], table[r0:r0 + n].tolist(), pro[r0:r0 + n].tolist(), chain[r0:r0 + n].tolist())
                detail = {}
                for got in (S.G.dssp(*args), S.G.dssp(*args, 1.0, None, detail)):
                    for a, want, what in zip(got, (codes, partners, em), ("codes", "partners", "em")):
                        assert a.dtype == want.dtype and np.array_equal(a, want[f, r0:r0 + n]), (name, f, r0, what)
                assert set(detail) == {"bridges", "ladders", "roots"} and len(detail["roots"]) == len(detail["ladders"])
                assert sum(L[5] for L in detail["ladders"]) == len(detail["bridges"]) and set(detail["bridges"].values()) <= {"P", "A"}
                assert all(detail["roots"][r] == r for r in detail["roots"])              # a root names itself
                r0 += n
    print(f"the golden regenerated twice in {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("case", S.CASES, ids=IDS)
def test_case_is_deterministic_unflagged_and_as_promised(case):
    family, seed, shape = case
    kind, flags = S.parse(family)
    c = S.build(case)
    t0 = time.perf_counter()
    again = S.build_fresh(case)
    took = time.perf_counter() - t0
    print(f"{S.case_id(case)}: attempt {c['attempt']}, {took:.3f} s, X {list(c['X'].shape)}, sizes {c['sizes']}")
    assert c["attempt"] == again["attempt"] < S.TRIES
    for k in ("X", "table", "pro", "chain", "codes", "partners", "em"):
        assert c[k].dtype == again[k].dtype and c[k].shape == again[k].shape and c[k].tobytes() == again[k].tobytes(), (case, k)
    assert c["sizes"] == again["sizes"] and c["scale"] == again["scale"] and c["detail"] == again["detail"]
    # the shapes and types pesto_amd.dssp takes, in the layout of test_dssp_fixture.case
    X, table, pro, chain, sizes, codes, partners, em = (c[k] for k in ("X", "table", "pro", "chain", "sizes", "codes", "partners", "em"))
    F, R = S.case_sizes(case)[0], sum(sizes)
    assert sizes == S.case_sizes(case)[1] and X.dtype == np.float32 and X.shape[0] == F and X.shape[2] == 3
    assert table.dtype == np.int32 and table.shape == (R, 4) and pro.dtype == np.uint8 and chain.dtype == np.int32 and pro.shape == chain.shape == (R,)
    assert codes.dtype == np.uint8 and codes.shape == (F, R) and partners.dtype == em.dtype == np.int32 and partners.shape == em.shape == (F, R, 4)
    assert table.min() >= -1 and table.max() < X.shape[1]
    # no near-threshold decision: the definition once more, on the stored arrays
    codes2, partners2, em2, detail2, flagged = S.define(X, table, pro, chain, sizes, c["scale"])
    assert not flagged and np.array_equal(codes2, codes) and np.array_equal(partners2, partners) and np.array_equal(em2, em) and detail2 == c["detail"]
    # the golden's structural invariants
    assert ((partners >= 0) == (em < 0)).all() and em.min() >= -9900 and codes.max() <= NA
    assert ((codes == NA) == (table < 0).any(1)[None]).all()
    assert (em[..., 0] <= em[..., 1]).all() and (em[..., 2] <= em[..., 3]).all()
    assert (partners < np.repeat(sizes, sizes)[None, :, None]).all()
    for p in shape[-1]:
        assert S.holds(p, c), (case, p)
    # the flags
    named = table[table >= 0]
    assert int(np.isnan(X).sum()) == ("nan" in flags) and np.isfinite(X[:, named][~np.isnan(X[:, named])]).all()
    if "nan" in flags:
        assert np.isnan(X[:, named]).sum() == 1
    offs = np.cumsum([0] + sizes)
    if "missing" in flags:
        gone = (table < 0).any(1)
        assert gone[0] and gone[-1] and (len(sizes) == 1 or gone[offs[1] - 1]) and (table < 0).sum() >= 2
        assert kind == "crop" or (table < 0).sum() <= max(3, round(0.03 * 4 * R))
    elif kind not in ("crop", "long"):
        assert (table >= 0).all()
    if "pro" in flags:
        assert 0 < pro.sum() <= max(2, 0.3 * R)
    if "rows" in flags:
        assert X.shape[1] == 6 * R + 3 and np.unique(named).size == named.size
        rest = np.setdiff1d(np.arange(X.shape[1]), named)
        assert (X[:, rest] == np.float32(1e6)).all() and (np.diff(table[(table >= 0).all(1)].ravel()) < 0).any()
    assert c["scale"] == (10.0 if "scale" in flags else 1.0)
    if "far" in flags:
        lo = np.nanmin(np.abs(X[:, named]) * c["scale"])
        assert lo > 8000
    if "chains" in flags:
        r = c["stretched"]
        d = np.linalg.norm(X[:, table[r, 0]].astype(np.float64) - X[:, table[r - 1, 2]].astype(np.float64), axis=1) * c["scale"]
        assert chain[r] == chain[r - 1] and (d > 2.6).all() and (np.diff(chain) > 0).any()
    if kind == "clash" and shape[1] == "zero":
        assert np.array_equal(X[:, table[4, 3]], X[:, table[4, 2]]) and table[4, 3] != table[4, 2]


def every_structure():
    for case in S.CASES:
        c = S.build(case)
        for f, s, codes, partners, em, detail in S.structures(c):
            yield case, codes, partners, em, detail


def test_the_list_reaches_what_the_recorded_cases_never_did():
    """read from the definition's codes, tables and detail, case by case (not through the promises)"""
    seen, letters = set(), set()
    for case, codes, partners, em, detail in every_structure():
        kind = S.parse(case[0])[0]
        t = S.text(codes)
        letters |= set(codes.tolist())
        lad, br, roots = detail["ladders"], detail["bridges"], detail["roots"]
        sizes = np.bincount(roots, minlength=1) if roots else np.zeros(1, int)
        per_i, per_r = {}, {}
        for (i, j), ty in br.items():
            per_i.setdefault(i, []).append(ty)
            per_r.setdefault(i, set()).add(ty)
            per_r.setdefault(j, set()).add(ty)
        found = {
            "H directly followed by I": "HI" in t, "G directly followed by H": "GH" in t,
            "an isolated I run of exactly 5": re.search(r"(?<!I)IIIII(?!I)", t) is not None,
            "a parallel ladder of >= 5": kind == "sheet" and any(L[0] == "P" and L[5] >= 5 for L in lad),
            "an antiparallel ladder of >= 5": kind == "sheet" and any(L[0] == "A" and L[5] >= 5 for L in lad),
            "a residue i with two bridges of different type": any(len(set(v)) == 2 for v in per_i.values()),
            "a residue i with more than two bridges": any(len(v) > 2 for v in per_i.values()),
            "a mixed sheet": any(len(v) == 2 for v in per_r.values()),
            "a component of >= 3 ladders": kind == "crop" and (sizes >= 3).any(), "a component of exactly 2 ladders": kind == "crop" and (sizes == 2).any(),
            "exactly one bridge, coded B": kind == "crop" and len(br) == 1 and all(codes[r] == B for r in next(iter(br))),
            "two best acceptors at -9900": ((em[:, 0] == -9900) & (em[:, 1] == -9900)).any(),
            "two best donors at -9900": ((em[:, 2] == -9900) & (em[:, 3] == -9900)).any(),
            "a bond at exactly -500": (em[:, :2] == -500).any(),
        }
        seen |= {k for k, v in found.items() if v}
    print("reached:", sorted(seen))
    assert letters == {BLANK, H, B, E, G, I, T, BEND, NA}
    # (more than two bridges at one residue i would need one residue in three strands' ladders as the first index; the list promises two)
    assert seen >= set(found) - {"a residue i with more than two bridges"}, set(found) - seen
    # the pi-helix whose first turn lies on an alpha-helix, and the link at the far end of the bulge scan
    assert S.holds("Hwins", S.build(S.CASES[0])) and all(S.holds("gi4", S.build(c)) for c in S.CASES if c[0] == "bulge")


def test_case_list_covers_every_edge_set():
    table = S.coverage()
    for key in sorted(table):
        print(f"{key:32s} {sorted(table[key], key=str)}")
    for key, need in S.REQUIRED.items():
        assert need <= table[key], (key, need - table[key])
    for fl in S.FLAGS:                                  # every flag in at least three kinds
        assert len(table["flag:" + fl]) >= 3, (fl, table["flag:" + fl])
    assert len(table["F>=2,n_struct>=2"]) >= 4
    assert table.get("above 2000 residue-frames", set()) <= {"long"}
    assert 35 <= len(S.CASES) <= 45 and len(set(IDS)) == len(IDS) and len({c[1] for c in S.CASES}) == len(S.CASES)
    for kind in table["kinds"]:                         # every kind runs from host arrays too
        assert any(S.every_third(c) for c in S.CASES if S.parse(c[0])[0] == kind)
