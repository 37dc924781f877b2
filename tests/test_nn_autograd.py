"""pesto_amd.nn.Model on the GPU: forward bits against pesto_amd.training.Trainer, the gradients of the parameters, the coordinates and
the input features against the reference's float64 autograd (tests/golden/make_autograd_golden.py), and the reference's training loop
(its loss restated with torch ops + torch.optim.Adam) against the recorded float64 loss curve.

Bounds: training_fixture.grad_bound - 8 x the reference's own float32-vs-float64 error of the case in the same metric, at most 1e-3."""
import numpy as np
import pytest
import torch

from conftest import golden, onehot
from pesto_amd import _lib
from training_fixture import CONFIG, KEYS, POS_WEIGHT_FACTOR, case, grad_bound, grad_error, split, state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_cache = {}


@pytest.fixture(scope="module")
def model():
    from pesto_amd.nn import Model
    m = Model(CONFIG)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_dict().items()})
    return m.to(DEV)


def inputs(name):
    """(X, ids_topk, q0, (res_of_atom, R)) as numpy arrays, and the recorded gradients of autograd_<name>.npz"""
    g = golden("autograd_" + name)
    if name == "D":
        roa = g["res_of_atom"].astype(np.int32)
        return (g["X"], g["ids_topk"].astype(np.int32), onehot(g["q_idx"][:, None], 30), (roa, int(roa.max()) + 1)), g
    return case(name)[0][:4], g


def on_device(batch, x_grad=False, q_grad=False):
    X, ids, q0, (roa, R) = batch
    X = torch.from_numpy(np.array(X, np.float32)).to(DEV).requires_grad_(x_grad)
    q = torch.from_numpy(q0).to(DEV).requires_grad_(q_grad)
    return X, torch.from_numpy(ids.astype(np.int64)).to(DEV), q, (torch.from_numpy(roa).to(DEV), R)


def backward(model, name, dz=None, x_grad=True, q_grad=True):
    """z and the gradients of sum(z * dz): ({key: array}, dX, dq0) (None where not asked for)"""
    batch, g = inputs(name)
    X, ids, q, M = on_device(batch, x_grad, q_grad)
    model.zero_grad(set_to_none=True)
    z = model(X, ids, q, M)
    (z * torch.from_numpy(g["dz"] if dz is None else dz).to(DEV)).sum().backward()
    grads = {k: p.grad.cpu().numpy() if p.grad is not None else None for k, p in model.named_parameters()}
    return z.detach().cpu().numpy(), grads, None if X.grad is None else X.grad.cpu().numpy(), None if q.grad is None else q.grad.cpu().numpy()


def full(model, name):
    """the case's backward with both input gradients, computed once and shared"""
    if name not in _cache:
        _cache[name] = backward(model, name)
    return _cache[name]


def check(err, bound, what):
    worst = max(err, key=err.get)
    print(f"{what}: worst E = {err[worst]:.3e} ({worst}), bound {bound:.3e}")
    bad = {k: v for k, v in err.items() if not v <= bound}
    assert not bad, (what, bound, bad)


# ------------------------------------------------------------------ 1. forward
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_forward_bits(model, name):
    from pesto_amd.training import Trainer
    batch, g = case(name)
    tr = Trainer(CONFIG, state_dict())
    tr.eval_step(*batch)
    z_tr = np.array(tr.last_z)
    tr.close()
    X, ids, q, M = on_device(batch[:4])
    z = model(X, ids, q, M)
    assert z.requires_grad and z.is_cuda
    with torch.no_grad():
        z_ng = model(X, ids, q, M)
    assert not z_ng.requires_grad
    print(f"case {name}: |z - golden| = {np.abs(z.detach().cpu().numpy() - g['z']).max():.2e}")
    assert np.array_equal(z.detach().cpu().numpy(), z_tr)
    assert np.array_equal(z_ng.cpu().numpy(), z_tr)
    assert np.abs(z_tr - g["z"]).max() <= 1e-4
    dense = torch.zeros((X.shape[0], M[1]), device=DEV)      # the reference's dense mask gives the same call
    dense[torch.arange(X.shape[0], device=DEV), M[0].long()] = 1.0
    with torch.no_grad():
        assert torch.equal(model(X, ids, q, dense), z_ng)


# ------------------------------------------------------------------ 2. parameter gradients
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_parameter_gradients(model, name):
    g = inputs(name)[1]
    _, grads, _, _ = full(model, name)
    check(grad_error(grads, split(g["grads"])), grad_bound(g["E_ref"]), f"case {name} parameters")


# ------------------------------------------------------------------ 3. input gradients
@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
def test_input_gradients(model, name):
    g = inputs(name)[1]
    _, _, dX, dq0 = full(model, name)
    assert np.isfinite(dX).all() and np.isfinite(dq0).all()
    if name != "B":
        assert int(g["n_fixup"]) > 0 and float(g["dm"]) != 0.0      # the fix-up's gradient is exercised
    check(grad_error({"dX": dX, "dq0": dq0}, {"dX": g["dX"], "dq0": g["dq0"]}), grad_bound(g["E_ref_inputs"]), f"case {name} inputs")


def test_collated_structures_are_independent(model):
    """case B, 200 + 70 atoms, no fix-up edge: what structure 1's residues receive does not reach structure 2's coordinates"""
    (batch, g), sizes = inputs("B"), case("B")[1]["sizes"]
    n1 = int(sizes[0])
    r1 = int(batch[3][0][n1 - 1]) + 1      # residues of structure 1
    _, _, dX, dq0 = full(model, "B")
    dz = g["dz"].copy()
    dz[:r1] = 0.0
    _, _, dX2, dq2 = backward(model, "B", dz=dz)
    assert np.array_equal(dX2[n1:], dX[n1:]) and np.array_equal(dq2[n1:], dq0[n1:])
    assert not dX2[:n1].any() and np.abs(dX[:n1]).max() > 0


# ------------------------------------------------------------------ 4. the geometry variant changes nothing else
def test_geometry_variant_and_retain_graph(model):
    _, grads, dX, dq0 = full(model, "A")
    _, grads_p, dX_p, dq_p = backward(model, "A", x_grad=False, q_grad=False)
    assert dX_p is None and dq_p is None
    for k in grads:
        assert np.array_equal(grads[k], grads_p[k]), k
    _, _, dX_x, dq_x = backward(model, "A", x_grad=True, q_grad=False)
    assert dq_x is None and np.array_equal(dX_x, dX)
    batch, g = inputs("A")
    X, ids, q, M = on_device(batch, True, True)
    z = model(X, ids, q, M)
    wrt = list(model.parameters()) + [X, q]
    dz = torch.from_numpy(g["dz"]).to(DEV)
    first = torch.autograd.grad(z, wrt, dz, retain_graph=True)
    second = torch.autograd.grad(z, wrt, dz)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    assert np.array_equal(first[-2].cpu().numpy(), dX) and np.array_equal(first[-1].cpu().numpy(), dq0)


# ------------------------------------------------------------------ 5. the reference's loop
def reference_loss(z, y, pos_ratios, global_step):
    """model/main.py:49-58 with torch ops (pos_ratios is updated in place, as there)"""
    pos_ratios += (torch.mean(y, dim=0).detach() - pos_ratios) / (1.0 + np.sqrt(global_step))
    criterion = torch.nn.BCEWithLogitsLoss(reduction="none")
    criterion.pos_weight = POS_WEIGHT_FACTOR * (1.0 - pos_ratios) / (pos_ratios + 1e-6)
    dloss = criterion(z, y)
    return ((pos_ratios / torch.sum(pos_ratios)).reshape(1, -1) * dloss) / dloss.shape[0]


def test_training_loop_matches_the_reference_curve():
    from pesto_amd.nn import Model
    g = golden("training_curve")
    roa = g["res_of_atom"].astype(np.int32)
    X, ids, q, M = on_device((g["X"], g["ids_topk"].astype(np.int32), onehot(g["q_idx"][:, None], 30), (roa, int(roa.max()) + 1)))
    y = torch.from_numpy(g["y"].astype(np.float32)).to(DEV)
    m = Model(CONFIG)
    m.load_state_dict({k: torch.from_numpy(np.array(v)) for k, v in state_dict().items()})
    m.to(DEV)
    optimizer = torch.optim.Adam(m.parameters(), lr=1e-3)
    pos = 0.5 * torch.ones(5, device=DEV)
    curve = []
    for step in range(1, 25):
        optimizer.zero_grad()
        loss = torch.sum(reference_loss(m(X, ids, q, M), y, pos, step))
        loss.backward()
        optimizer.step()
        curve.append(float(loss.detach()))
    curve = np.array(curve)
    dev = np.abs(curve - g["loss64"]).max()
    print("curve", np.round(curve, 4), f"max deviation {dev:.3e}, bound {100 * float(g['deviation']):.3e}")
    assert dev <= 100 * float(g["deviation"])
    assert curve[-1] < 0.7 * curve.max()
    sd = m.state_dict()      # what torch.save would write: the reference's keys, and the fast inference model takes it
    z_fast = m.inference_model(precision="fp32").forward_segments(g["X"], g["ids_topk"].astype(np.int32), onehot(g["q_idx"][:, None], 30), roa, int(roa.max()) + 1)
    with torch.no_grad():
        assert np.abs(m(X, ids, q, M).cpu().numpy() - z_fast).max() <= 1e-4
    assert set(sd) >= {k for k, _ in KEYS}


# ------------------------------------------------------------------ 6. frozen subset
def test_frozen_subset(model):
    _, grads, _, _ = full(model, "C")
    model.em.requires_grad_(False)
    try:
        _, frozen, dX, _ = backward(model, "C")
    finally:
        model.em.requires_grad_(True)
    for k, v in frozen.items():
        if k.startswith("em."):
            assert v is None, k
        else:
            assert np.array_equal(v, grads[k]), k
    assert np.array_equal(dX, full(model, "C")[2])


# ------------------------------------------------------------------ 7. / 8. failures
def test_stale_ticket(model):
    batch, g = inputs("A")
    X, ids, q, M = on_device(batch)
    z1 = model(X, ids, q, M)
    z2 = model(X, ids, q, M)
    with pytest.raises(RuntimeError, match="not the handle's last kept forward"):
        z1.sum().backward()
    z2.sum().backward()      # the last forward's own backward is fine
    z3 = model(X, ids, q, M)
    with torch.no_grad():
        model(X, ids, q, M)      # a forward without gradient runs on the same workspace
    with pytest.raises(RuntimeError, match="not the handle's last kept forward"):
        z3.sum().backward()
    _, grads, _, _ = backward(model, "A")      # and the model works afterwards
    for k, v in full(model, "A")[1].items():
        assert np.array_equal(grads[k], v), k


def test_argument_errors(model):
    batch, g = inputs("A")
    X, ids, q, M = on_device(batch)
    before = {k: v.clone() for k, v in model.state_dict().items()}
    bad = ids.clone(); bad[3, 2] = X.shape[0] + 1
    with pytest.raises(_lib.PestoError, match="ids_topk"):
        model(X, bad, q, M)
    neg = ids.clone(); neg[0, 0] = -1
    with pytest.raises(_lib.PestoError, match="ids_topk"):
        with torch.no_grad():
            model(X, neg, q, M)
    with pytest.raises(_lib.PestoError, match="no atom"):
        model(X, ids, q, (M[0], M[1] + 1))
    with pytest.raises(_lib.PestoError, match="float32"):
        model(X.double(), ids, q, M)
    with pytest.raises(_lib.PestoError, match="GPU"):
        model(X.cpu(), ids, q, M)
    for k, v in model.state_dict().items():
        assert torch.equal(v, before[k]), k
    z, _, _, _ = backward(model, "A")
    assert np.array_equal(z, full(model, "A")[0])
