"""pesto_amd.training and pesto_amd.nn on the GPU at the launch-shape edges of pesto_train.hip (the cases of tests/training_sweep.py) against
the float64 run of the definition (tests/model_def.py, pinned to the recorded fixtures by tests/test_training_sweep_fixture.py).

Bounds: training_sweep.bound - min(1e-3, 8 x max(E_ref(case), E_floor)) in the suite's metric, E_ref the definition's own float32-vs-float64
error of the case and E_floor the smallest such error the committed fixtures record (autograd_B); logits at the project's forward bound
1e-4; losses and pos_ratios at 1e-6 x max(1, max|value|). A second run, the other id type, the dense mask, ROCm tensors (every third
case) and x_grad=False give the same bits."""
import numpy as np
import pytest
import torch

import training_sweep as S
from pesto_amd.weights import flatten_state_dict, unflatten_blob
from training_fixture import grad_error

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
WORST = {}      # (model, what) -> (worst E, worst E / bound) of the run, printed by the last test


class Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, name):
        self[name] = self.make(name)
        return self[name]


@pytest.fixture(scope="module")
def trainers():
    from pesto_amd.training import Trainer
    made = Lazy(lambda name: Trainer(*S.model(name)))
    yield made
    for tr in made.values():
        tr.close()


@pytest.fixture(scope="module")
def modules():
    from pesto_amd.nn import Model

    def make(name):
        cfg, sd = S.model(name)
        m = Model(cfg)
        m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in unflatten_blob(cfg, flatten_state_dict(cfg, sd)).items()})
        return m.to(DEV)
    return Lazy(make)


def check(model, what, case, g, ref, bound):
    err = grad_error(g, ref)
    e, k = S.worst(err)
    print(f"{S.case_id(case)} {what}: worst E = {e:.3e} ({k}), bound {bound:.3e}")
    w = WORST.get((model, what), (0.0, 0.0))
    WORST[(model, what)] = (max(w[0], e), max(w[1], e / bound))
    bad = {k: v for k, v in err.items() if not v <= bound}
    assert not bad, (S.case_id(case), what, bound, bad)


def near(what, case, got, want, tol):
    dev = float(np.abs(np.asarray(got, np.float64) - want).max())
    print(f"{S.case_id(case)} {what}: max deviation {dev:.3e}, bound {tol:.3e}")
    assert dev <= tol, (S.case_id(case), what, dev, tol)


def same(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


def other(ids, ids_as):
    return ids.astype(np.int32 if ids_as == "i64" else np.int64)


def dense(roa, R):
    M = np.zeros((roa.size, R), np.float32)
    M[np.arange(roa.size), roa] = 1.0
    return M


# ------------------------------------------------------------------ 1. loss_and_grad
@pytest.mark.parametrize("case", S.STEP, ids=S.case_id)
def test_loss_and_grad(trainers, case):
    b = S.build("step", case)
    name = case[0]
    tr = trainers[name]
    C = tr.config["dm"]["N2"]
    blob0 = tr.blob()
    X, q0, roa, R, y, ref = b["X"], b["q0"], b["roa"], b["R"], b["y"], b["s64"]
    ids = b["ids"].astype(np.int64 if b["ids_as"] == "i64" else np.int32)

    def run(ids, M, to=lambda a: a):
        tr.pos_ratios = np.full(C, 0.5, np.float32)
        tr.global_step = b["step"]
        losses, p, grads = tr.loss_and_grad(to(X), to(ids), to(q0), M, to(y))
        host = lambda a: a.cpu().numpy() if torch.is_tensor(a) else np.array(a)      # noqa: E731
        out = dict({k: host(v) for k, v in grads.items()}, losses=host(losses), p=host(p), pos=tr.pos_ratios, z=host(tr.last_z))
        assert tr.global_step == b["step"]
        return out

    got = run(ids, (roa, R))
    check(name, "loss_and_grad", case, got, ref["grads"], S.bound("parameters", b["e_ref"]["step"][0]))
    near("last_z", case, got["z"], ref["z"], 1e-4)
    near("p", case, got["p"], ref["p"], 1e-4)
    near("losses", case, got["losses"], ref["losses"], 1e-6 * max(1.0, float(np.abs(ref["losses"]).max())))
    near("pos_ratios", case, got["pos"], ref["pos"], 1e-6 * max(1.0, float(np.abs(ref["pos"]).max())))
    same(got, run(ids, (roa, R)), "second run")
    same(got, run(other(ids, b["ids_as"]), (roa, R)), "the other id type")
    same(got, run(ids, dense(roa, R)), "dense mask")
    if S.every_third("step", case):
        same(got, run(ids, (torch.from_numpy(roa).to(DEV), R), lambda a: torch.from_numpy(a).to(DEV)), "ROCm tensors")
    assert np.array_equal(tr.blob(), blob0)      # no update


# ------------------------------------------------------------------ 2. nn.Model's backward from a seeded dz
def module_backward(model, b, ids, M, dz, x_grad=True):
    X = torch.from_numpy(b["X"]).to(DEV).requires_grad_(x_grad)
    q = torch.from_numpy(b["q0"]).to(DEV).requires_grad_(x_grad)
    model.zero_grad(set_to_none=True)
    z = model(X, torch.from_numpy(ids).to(DEV), q, M)
    (z * torch.from_numpy(dz).to(DEV)).sum().backward()
    out = {k: p.grad.cpu().numpy() for k, p in model.named_parameters()}
    if x_grad:
        out.update(dX=X.grad.cpu().numpy(), dq0=q.grad.cpu().numpy())
    return dict(out, z=z.detach().cpu().numpy())


@pytest.mark.parametrize("case", S.STEP, ids=S.case_id)
def test_module_backward(modules, case):
    b = S.build("step", case)
    name = case[0]
    m = modules[name]
    roa, R, ref = b["roa"], b["R"], b["a64"]
    ids = b["ids"].astype(np.int64 if b["ids_as"] == "i64" else np.int32)
    M = (torch.from_numpy(roa).to(DEV), R)
    got = module_backward(m, b, ids, M, b["dz"])
    check(name, "nn parameters", case, got, ref["grads"], S.bound("parameters", b["e_ref"]["parameters"][0]))
    check(name, "nn inputs", case, got, dict(dX=ref["dX"], dq0=ref["dq0"]), S.bound("inputs", b["e_ref"]["inputs"][0]))
    near("z", case, got["z"], ref["z"], 1e-4)
    same(got, module_backward(m, b, ids, M, b["dz"]), "second run")
    same(got, module_backward(m, b, other(ids, b["ids_as"]), M, b["dz"]), "the other id type")
    same(got, module_backward(m, b, ids, torch.from_numpy(dense(roa, R)).to(DEV), b["dz"]), "dense mask")
    same(module_backward(m, b, ids, M, b["dz"], x_grad=False), got, "x_grad=False")


def test_collated_structures_are_independent(modules):
    """every structure has more than 64 + 1 atoms and the batch no fix-up edge: what structure 1's residues receive reaches nothing else"""
    case = S.INDEPENDENT
    b = S.build("step", case)
    m = modules[case[0]]
    n1 = case[2][0][0]
    r1 = int(b["roa"][:n1].max()) + 1
    assert b["roa"][n1:].min() == r1
    ids, M = b["ids"].astype(np.int64), (torch.from_numpy(b["roa"]).to(DEV), b["R"])
    full = module_backward(m, b, ids, M, b["dz"])
    dz = b["dz"].copy()
    dz[:r1] = 0.0
    part = module_backward(m, b, ids, M, dz)
    assert np.array_equal(part["dX"][n1:], full["dX"][n1:]) and np.array_equal(part["dq0"][n1:], full["dq0"][n1:])
    assert not part["dX"][:n1].any() and not part["dq0"][:n1].any() and np.abs(full["dX"][:n1]).max() > 0


# ------------------------------------------------------------------ 3. the stage entry points
def outside_is_zero(name, grads, prefixes):
    for k, _ in S.keys(name):
        if not k.startswith(prefixes):
            assert not grads[k].any(), k


@pytest.mark.parametrize("case", S.LAYER, ids=S.case_id)
def test_stage_layer(trainers, case):
    b = S.build("layer", case)
    name, l = case[0], case[2][0]
    dq, dp, grads = trainers[name].stage_layer_bwd(*b["args"])
    ref = b["r64"]
    check(name, f"layer {l} weights", case, grads, ref["grads"], S.bound("parameters", b["e_ref"]["parameters"][0]))
    check(name, f"layer {l} states", case, dict(dq_in=dq[1:], dp_in=dp[1:]), dict(dq_in=ref["dq_in"][1:], dp_in=ref["dp_in"][1:]),
          S.bound("inputs", b["e_ref"]["inputs"][0]))
    outside_is_zero(name, grads, f"sum.{l}.")
    dq2, dp2, grads2 = trainers[name].stage_layer_bwd(*b["args"])
    same(dict(grads, dq=dq, dp=dp), dict(grads2, dq=dq2, dp=dp2), "second run")


@pytest.mark.parametrize("case", S.HEAD, ids=S.case_id)
def test_stage_head(trainers, case):
    b = S.build("head", case)
    name = case[0]
    dq, dp, grads = trainers[name].stage_head_bwd(*b["args"])
    ref = b["r64"]
    check(name, "head weights", case, grads, ref["grads"], S.bound("parameters", b["e_ref"]["parameters"][0]))
    check(name, "head states", case, dict(dq=dq, dp=dp), dict(dq=ref["dq"], dp=ref["dp"]), S.bound("inputs", b["e_ref"]["inputs"][0]))
    outside_is_zero(name, grads, ("spl.", "dm."))
    dq2, dp2, grads2 = trainers[name].stage_head_bwd(*b["args"])
    same(dict(grads, dq=dq, dp=dp), dict(grads2, dq=dq2, dp=dp2), "second run")


@pytest.mark.parametrize("case", S.EMBED, ids=S.case_id)
def test_stage_embed(trainers, case):
    b = S.build("embed", case)
    name = case[0]
    grads = trainers[name].stage_embed_bwd(*b["args"])
    check(name, "embed weights", case, grads, b["r64"]["grads"], S.bound("parameters", b["e_ref"]["parameters"][0]))
    outside_is_zero(name, grads, "em.")
    same(grads, trainers[name].stage_embed_bwd(*b["args"]), "second run")


def test_report_worst():
    """the worst E and the worst E / bound per model and comparison of this run (DESIGN.md 4.15 / 4.16 quote them)"""
    print()
    for (model, what), (e, share) in sorted(WORST.items()):
        print(f"worst {model} {what}: E = {e:.3e}, E / bound = {share:.3f}")
