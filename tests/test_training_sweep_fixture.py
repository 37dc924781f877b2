"""CPU checks of the training sweep (tests/training_sweep.py, tests/model_def.py): the definition reproduces, in float64, every gradient the
repository records from the reference (training_{A,B,C}, autograd_{A,B,C,D}, training_stage_L{0..3}, training_stage_head) within 2^-22 in
the suite's metric - the recorded values are float64 results rounded to float32, 2^-24 relative to an entry and so at most that in the
metric, and a factor of 4 covers float64 summation order; the case lists cover every edge set; every builder promise holds; the seeded
weights are the recorded ones; E_ref of every case keeps 8 x E_ref below the bound's cap."""
import numpy as np
import pytest

import training_sweep as S
from conftest import golden
from test_nn_autograd import inputs as autograd_inputs
from training_fixture import KEYS, case, grad_error, split

E_PIN = 2.0 ** -22
ALL = S.all_cases()
IDS = [f"{entry}:{S.case_id(c)}" for entry, c in ALL]


def pinned(what, g, ref):
    e, k = S.worst(grad_error(g, ref))
    print(f"{what}: worst E = {e:.3e} ({k}), bound {E_PIN:.3e}")
    assert e <= E_PIN, (what, k, e)
    return e


def d64():
    return S.definition("M4", 64)


# ------------------------------------------------------------------ 1. the definition against the thirteen recorded files
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_definition_reproduces_training(name):
    (X, ids, q0, (roa, R), y), g = case(name)
    r = S.step_def(d64(), X, ids, q0, roa, R, y, 0)
    e = pinned(f"training_{name} grads", r["grads"], split(g["grads"]))
    print(f"training_{name}: worst E {e:.3e} |z - ref| = {np.abs(r['z'] - g['z']).max():.2e} |losses - ref| = {np.abs(r['losses'] - g['losses']).max():.2e}")
    assert np.abs(r["z"] - g["z"]).max() <= 1e-4
    assert np.abs(r["losses"] - g["losses"]).max() <= 1e-6 and np.abs(r["pos"] - g["pos_ratios"]).max() <= 1e-6
    r1 = S.step_def(d64(), X, ids, q0, roa, R, y, 1)
    assert np.abs(r1["losses"] - g["losses_step1"]).max() <= 1e-6 and np.abs(r1["pos"] - g["pos_ratios_step1"]).max() <= 1e-6


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_definition_reproduces_autograd(name):
    (X, ids, q0, (roa, R)), g = autograd_inputs(name)
    r = S.autograd_def(d64(), X, ids, q0, roa, R, g["dz"])
    e = max(pinned(f"autograd_{name} grads", r["grads"], split(g["grads"])),
            pinned(f"autograd_{name} inputs", dict(dX=r["dX"], dq0=r["dq0"]), dict(dX=g["dX"], dq0=g["dq0"])))
    print(f"autograd_{name}: worst E {e:.3e} |z - ref| = {np.abs(r['z'] - g['z']).max():.2e} fix-up edges {r['n_fixup']} d max = {r['dm']:.3e}")
    assert np.abs(r["z"] - g["z"]).max() <= 1e-4
    assert r["n_fixup"] == int(g["n_fixup"]) and abs(r["dm"] - float(g["dm"])) <= E_PIN * max(1.0, abs(float(g["dm"])))


@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_definition_reproduces_stage_layer(layer):
    (X, ids, _, _, _), _ = case("B")
    g = golden(f"training_stage_L{layer}")
    r = S.layer_def(d64(), layer, X, ids, g["q_in"], g["p_in"], g["dq_out"], g["dp_out"])
    e = max(pinned(f"stage L{layer} grads", r["grads"], split(g["grads"], [(k, s) for k, s in KEYS if k.startswith(f"sum.{layer}.")])),
            pinned(f"stage L{layer} states", dict(dq_in=r["dq_in"][1:], dp_in=r["dp_in"][1:]), dict(dq_in=g["dq_in"][1:], dp_in=g["dp_in"][1:])))
    print(f"training_stage_L{layer}: worst E {e:.3e}")


def test_definition_reproduces_stage_head():
    (_, _, q0, (roa, R), _), _ = case("B")
    g = golden("training_stage_head")
    r = S.head_def(d64(), g["q"], g["p"], roa, R, g["dz"])
    e = max(pinned("stage head grads", r["grads"], split(g["grads_head"], [(k, s) for k, s in KEYS if k.startswith(("spl.", "dm."))])),
            pinned("stage head states", dict(dq=r["dq"], dp=r["dp"]), dict(dq=g["dq"], dp=g["dp"])),
            pinned("stage embed grads", S.embed_def(d64(), q0, g["dq_em"])["grads"], split(g["grads_em"], [(k, s) for k, s in KEYS if k.startswith("em.")])))
    print(f"training_stage_head: worst E {e:.3e}")


# ------------------------------------------------------------------ 2. the case lists
def test_case_lists_cover_every_edge_set():
    table = S.coverage()
    for key in sorted(table, key=str):
        print(f"{key[0]:6s} {key[1]:24s} {sorted(table[key], key=str)}")
    print("cases per list:", {k: len(v) for k, v in S.CASES.items()})
    for key, need in S.REQUIRED.items():
        assert need <= table[key], (key, need - table[key])
    ids = [S.case_id(c) for _, c in ALL]
    assert len(set(ids)) == len(ids) and len({c[1] for _, c in ALL}) == len(ALL)      # every case a name and a seed of its own
    assert not any(sum(c[2][0]) == 1 for c in S.STEP)      # N = 1: its only edge has length 0 and a fix-up of 0
    assert all(any(S.every_third(e, c) for c in cases) for e, cases in S.CASES.items())
    assert min(S.INDEPENDENT[2][0]) > 64 + 1 and len(S.INDEPENDENT[2][0]) >= 2


def test_seeded_weights_are_the_recorded_ones():
    for name in ("R1", "R2"):
        cfg, sd = S.model(name)
        digest = S.blob_sha256(cfg, sd)
        print(name, digest)
        assert digest == S.SEEDED_SHA256[name], name
    assert S.model("M3")[0]["em"]["N0"] == 123 and S.model("R2")[0]["em"]["N0"] == 512 and S.model("R1")[0]["dm"]["N2"] == 1


def test_floor_is_the_smallest_recorded_error():
    for kind, field in (("parameters", "E_ref"), ("inputs", "E_ref_inputs")):
        recorded = [float(golden(f"autograd_{n}")[field]) for n in "ABCD"]
        print(kind, recorded)
        assert S.e_floor(kind) == min(recorded)


# ------------------------------------------------------------------ 3. the builders' promises, and E_ref per case
@pytest.mark.parametrize("entry,c", ALL, ids=IDS)
def test_case_keeps_its_promises(entry, c):
    b = S.build(entry, c)
    print(f"{entry} {S.case_id(c)}: attempt {b['attempt']} " + " ".join(f"E_ref({k}) = {e:.3e} ({t})" for k, (e, t) in b["e_ref"].items()))
    assert all(8.0 * e < 1e-3 for e, _ in b["e_ref"].values())
    if entry == "step":
        sizes, layout, k, ids_as, ymode, step = c[2]
        X, ids, roa, R, y = b["X"], b["ids"], b["roa"], b["R"], b["y"]
        assert X.dtype == np.float32 and ids.dtype == np.int32 and ids.shape == (sum(sizes), k) and ids.min() >= 0 and ids.max() <= X.shape[0]
        assert np.array_equal(np.unique(roa), np.arange(R)) and y.shape == (R, S.model(c[0])[0]["dm"]["N2"])
        clear, maximal = S.geometry_facts(X, ids)
        assert clear and (len(maximal) == 1 or (len(maximal) == 2 and maximal[0] == maximal[1][::-1])), maximal
        for r in (b["s64"], b["a64"]):
            assert all(np.isfinite(v).all() for v in r["grads"].values())
        assert np.isfinite(b["a64"]["dX"]).all() and np.isfinite(b["a64"]["dq0"]).all() and np.abs(b["a64"]["dX"]).max() > 0
        if ymode == "zero":
            assert not y[:, 0].any()
        if ymode == "one":
            assert y[:, -1].all()
        if min(sizes) > k + 1:
            assert b["a64"]["n_fixup"] == 0 and (ids > 0).all()
        R0, largest, interleaved = S.layout_facts(sizes, layout, c[1])
        assert layout == "mixed" or (not interleaved and (R0, largest) == (R, int(np.bincount(roa).max())))
    elif entry == "layer":
        l, N = c[2]
        assert b["args"][1].shape == (N, 3) and not b["args"][3][0].any() and not b["args"][4][0].any()
    elif entry == "head":
        N, layout = c[2]
        assert np.array_equal(np.unique(b["args"][2]), np.arange(b["args"][3]))


def test_mixed_layouts_interleave_and_fixups_reach_the_maximum():
    """the pool's roa[i] == r filter is exercised: some mixed case has atoms of two residues interleaved and a residue above 8 atoms; and
    every model has a whole-step case with a fix-up edge whose gradient reaches max D0"""
    mixed = [c for c in S.STEP if c[2][1] == "mixed"] + [(m, s, ((n,), lay)) for m, s, (n, lay) in S.HEAD if lay == "mixed"]
    facts = [np.bincount(S.build("step", c)["roa"]).max() for c in S.STEP if c[2][1] == "mixed"]
    assert any(S.layout_facts(c[2][0], "mixed", c[1])[2] for c in mixed) and max(facts) > 1
    for name in ("M4", "M3", "R1", "R2"):
        hits = [S.case_id(c) for c in S.STEP if c[0] == name and S.build("step", c)["a64"]["n_fixup"] > 0 and S.build("step", c)["a64"]["dm"] != 0.0]
        print(name, "fix-up gradient reaches max D0 in", hits)
        assert hits, name
