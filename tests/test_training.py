"""pesto_amd.training on the GPU against the reference's training step recorded by tests/golden/make_training_golden.py (float64 gradients,
float32 logits and losses) and, for Adam, against torch.optim.Adam run on the CPU in float64."""
import numpy as np
import pytest

from conftest import golden
from pesto_amd import _lib
from training_fixture import CONFIG, KEYS, case, grad_bound, grad_error, split, state_dict

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def trainer():
    from pesto_amd.training import Trainer
    tr = Trainer(CONFIG, state_dict())
    yield tr
    tr.close()


def fresh(lr=1e-5):
    from pesto_amd.training import Trainer
    return Trainer(CONFIG, state_dict(), lr=lr)


def check_grads(g, ref, bound, what):
    err = grad_error(g, ref)
    worst = max(err, key=err.get)
    print(f"{what}: worst E = {err[worst]:.3e} ({worst}), bound {bound:.3e}")
    bad = {k: v for k, v in err.items() if not v <= bound}
    assert not bad, (what, bound, bad)


def stage_keys(prefixes):
    return [(k, s) for k, s in KEYS if k.startswith(prefixes)]


# ------------------------------------------------------------------ 1. stage backward (case B's states)
@pytest.mark.parametrize("layer", [0, 1, 2, 3])
def test_stage_layer_backward(trainer, layer):
    (X, ids, _, _, _), gB = case("B")
    g = golden(f"training_stage_L{layer}")
    dq, dp, grads = trainer.stage_layer_bwd(layer, X, ids, g["q_in"], g["p_in"], g["dq_out"], g["dp_out"])
    keys = stage_keys(f"sum.{layer}.")
    ref = split(g["grads"], keys)
    bound = grad_bound(gB["E_ref"])
    check_grads({k: grads[k] for k in ref}, ref, bound, f"layer {layer} weights")
    # rows 1..N of the state gradients (what the gather sends to the sink row dies there, model_operations.py:239-240)
    check_grads({"dq_in": dq[1:], "dp_in": dp[1:]}, {"dq_in": g["dq_in"][1:], "dp_in": g["dp_in"][1:]}, bound, f"layer {layer} states")
    for k, s in KEYS:      # nothing outside the stage
        if not k.startswith(f"sum.{layer}."):
            assert not grads[k].any(), k


def test_stage_head_backward(trainer):
    (_, _, _, (roa, R), _), gB = case("B")
    g = golden("training_stage_head")
    dq, dp, grads = trainer.stage_head_bwd(g["q"], g["p"], roa, R, g["dz"])
    ref = split(g["grads_head"], stage_keys(("spl.", "dm.")))
    bound = grad_bound(gB["E_ref"])
    check_grads({k: grads[k] for k in ref}, ref, bound, "pool + dm weights")
    check_grads({"dq": dq, "dp": dp}, {"dq": g["dq"], "dp": g["dp"]}, bound, "pool + dm states")


def test_stage_embed_backward(trainer):
    (_, _, q0, _, _), gB = case("B")
    g = golden("training_stage_head")
    grads = trainer.stage_embed_bwd(q0, g["dq_em"])
    ref = split(g["grads_em"], stage_keys("em."))
    check_grads({k: grads[k] for k in ref}, ref, grad_bound(gB["E_ref"]), "embed weights")


# ------------------------------------------------------------------ 2. whole loss_and_grad
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_loss_and_grad(name):
    batch, g = case(name)
    tr = fresh()
    losses, p, grads = tr.loss_and_grad(*batch)
    pos, z = tr.pos_ratios, tr.last_z
    print(f"case {name}: |z - ref| = {np.abs(z - g['z']).max():.2e} |losses - ref| = {np.abs(losses - g['losses']).max():.2e} "
          f"|pos - ref| = {np.abs(pos - g['pos_ratios']).max():.2e}")
    l2, y2, p2 = tr.eval_step(*batch)      # the same state again, without gradient
    assert np.array_equal(p2, p) and np.array_equal(y2, batch[4])
    assert np.abs(z - g["z"]).max() <= 1e-4      # the project's forward bound
    assert np.abs(p - 1 / (1 + np.exp(-g["z"].astype(np.float64)))).max() <= 1e-4
    assert np.abs(losses - g["losses"]).max() <= 1e-6
    assert np.abs(pos - g["pos_ratios"]).max() <= 1e-6
    assert tr.global_step == 0
    assert np.array_equal(tr.blob(), np.concatenate([np.asarray(state_dict()[k], np.float32).ravel() for k, _ in KEYS]))      # no update
    check_grads(grads, split(g["grads"]), grad_bound(g["E_ref"]), f"case {name}")
    tr.close()


# ------------------------------------------------------------------ 3. Adam alone
def adam_bound(w, lr):
    return 4 * np.spacing(np.abs(w).astype(np.float32)).astype(np.float64) + 1e-5 * lr


def torch_adam(w0, grads, lr):
    import torch
    w = torch.nn.Parameter(torch.from_numpy(np.asarray(w0, np.float64).copy()))
    opt = torch.optim.Adam([w], lr=lr)
    for g in grads:
        opt.zero_grad()
        w.grad = torch.from_numpy(np.asarray(g, np.float64).copy())
        opt.step()
    return w.detach().numpy()


def test_adam_alone():
    lr = 1e-3
    tr = fresh(lr=lr)
    w0 = tr.blob()
    rng = np.random.default_rng(11)
    grads = [(rng.standard_normal(w0.size) * 10.0 ** rng.uniform(-6, 1, w0.size)).astype(np.float32) for _ in range(3)]
    for g in grads:
        tr.adam_step(g)
    w = tr.blob()
    ref = torch_adam(w0, grads, lr)
    err = np.abs(w.astype(np.float64) - ref)
    print(f"Adam: max error {err.max():.3e}, max error / bound {(err / adam_bound(ref, lr)).max():.3f}")
    assert (err <= adam_bound(ref, lr)).all()
    assert np.abs(w - w0).max() > 0.5 * lr
    # the plain section of the device image follows the blob: the forward sees the new weights
    batch, _ = case("A")
    _, _, p_new = tr.eval_step(*batch)
    tr2 = fresh()
    _, _, p_old = tr2.eval_step(*batch)
    assert np.abs(p_new - p_old).max() > 1e-4
    m = tr.model(precision="fp32")
    X, ids, q0, (roa, R), _ = batch
    z = m.forward_segments(X, ids, q0, roa, R)
    assert np.abs(1 / (1 + np.exp(-z.astype(np.float64))) - p_new).max() <= 1e-4
    tr.close(); tr2.close()


# ------------------------------------------------------------------ 4. train_step consistency
def test_train_step_consistency():
    batch, g = case("A")
    lr = 1e-3
    a = fresh(lr=lr)
    a.global_step = 1      # the state train_step computes its loss in
    losses_a, _, grads = a.loss_and_grad(*batch)
    b = fresh(lr=lr)
    w0 = b.blob()
    losses_b, y, p = b.train_step(*batch)
    assert b.global_step == 1
    assert np.abs(losses_b - losses_a).max() <= 1e-6 and np.abs(losses_b - g["losses_step1"]).max() <= 1e-6
    assert np.abs(b.pos_ratios - g["pos_ratios_step1"]).max() <= 1e-6
    flat = np.concatenate([grads[k].ravel() for k, _ in KEYS])
    ref = torch_adam(w0, [flat], lr)
    # every entry, the five tensors whose gradient is rounding noise included: there Adam turns the noise's sign into a full lr step, so
    # the two runs must have produced the same noise (the cross-workgroup sums are order-independent)
    err = np.abs(b.blob().astype(np.float64) - ref)
    tol = adam_bound(ref, lr)
    print(f"train_step: entries above the Adam bound {(err > tol).sum()} of {err.size}, max error {err.max():.3e}")
    assert (err <= tol).all()
    a.close(); b.close()


# ------------------------------------------------------------------ 5. loss curve
def test_loss_curve():
    g = golden("training_curve")
    from conftest import onehot
    roa = g["res_of_atom"].astype(np.int32)
    batch = (g["X"], g["ids_topk"].astype(np.int32), onehot(g["q_idx"][:, None], 30), (roa, int(roa.max()) + 1), g["y"].astype(np.float32))
    tr = fresh(lr=1e-3)
    curve = np.array([float(tr.train_step(*batch)[0].astype(np.float64).sum()) for _ in range(24)])
    dev = np.abs(curve - g["loss64"]).max()
    print("curve", np.round(curve, 4), f"max deviation {dev:.3e}, bound {100 * float(g['deviation']):.3e}")
    assert tr.global_step == 24
    assert dev <= 100 * float(g["deviation"])
    assert curve[-1] < 0.7 * curve.max()
    tr.close()


# ------------------------------------------------------------------ 6. argument errors
def test_argument_errors(trainer):
    batch, g = case("A")
    X, ids, q0, (roa, R), y = batch
    w0, pos0 = trainer.blob(), trainer.pos_ratios
    bad_ids = ids.copy(); bad_ids[3, 2] = X.shape[0] + 1
    with pytest.raises(_lib.PestoError, match="ids_topk"):
        trainer.train_step(X, bad_ids, q0, (roa, R), y)
    neg = ids.copy(); neg[0, 0] = -1
    with pytest.raises(_lib.PestoError, match="ids_topk"):
        trainer.loss_and_grad(X, neg, q0, (roa, R), y)
    with pytest.raises(_lib.PestoError, match="no atom"):      # an empty residue
        trainer.train_step(X, ids, q0, (roa, R + 1), np.zeros((R + 1, 5), np.float32))
    bad_roa = roa.copy(); bad_roa[5] = R
    with pytest.raises(_lib.PestoError, match="res_of_atom"):
        trainer.train_step(X, ids, q0, (bad_roa, R), y)
    with pytest.raises(_lib.PestoError):                         # y of the wrong shape
        trainer.train_step(X, ids, q0, (roa, R), y[:-1])
    with pytest.raises(_lib.PestoError, match="n_out"):          # n_out != C
        trainer.train_step(X, ids, q0, (roa, R), y[:, :4])
    # nothing moved, and the trainer works afterwards
    assert np.array_equal(trainer.blob(), w0) and np.array_equal(trainer.pos_ratios, pos0)
    step0 = trainer.global_step
    pos_before = trainer.pos_ratios
    losses, _, grads = trainer.loss_and_grad(*batch)
    assert trainer.global_step == step0 and np.isfinite(losses).all() and all(np.isfinite(v).all() for v in grads.values())
    trainer.pos_ratios = pos_before


def test_device_tensors_match_host_arrays():
    import torch
    batch, g = case("C")
    X, ids, q0, (roa, R), y = batch
    tr = fresh()
    dev = torch.device("cuda:0")
    M = torch.zeros((X.shape[0], R), device=dev)
    M[torch.arange(X.shape[0]), torch.from_numpy(roa.astype(np.int64))] = 1.0
    losses, p, grads = tr.loss_and_grad(torch.from_numpy(X).to(dev), torch.from_numpy(ids.astype(np.int64)).to(dev), torch.from_numpy(q0).to(dev), M,
                                        torch.from_numpy(y).to(dev))
    assert losses.is_cuda and p.is_cuda
    assert np.abs(losses.cpu().numpy() - g["losses"]).max() <= 1e-6
    check_grads({k: v.cpu().numpy() for k, v in grads.items()}, split(g["grads"]), grad_bound(g["E_ref"]), "case C, ROCm tensors")
    from pesto_amd.training import scoring
    s = scoring([(losses, torch.from_numpy(y).to(dev), p)])
    assert abs(s["loss"] - float(g["losses"].sum())) <= 1e-5 and "0/auc" in s
    tr.close()
