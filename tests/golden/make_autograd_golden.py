#!/usr/bin/env python3
"""Generate tests/golden/autograd_{A,B,C,D}.npz: the reference's gradients of sum(z * dz) with respect to the parameters, the coordinates
X and the input features q0, on its PyTorch CPU path in float32 and float64, for pesto_amd.nn. The reference is IMPORTED
(make_golden.import_reference); what is committed is data plus this script.

Model: the four-layer model of make_training_golden.py (trained i_v4_0, layers 0 / 4 / 8 / 12).
Inputs: A, B and C are the inputs of training_{A,B,C}.npz. D is B's first structure (N = 200) with atom 1 moved to 5e-3 A from atom 0
(topology recomputed): fix-up edges (D < 1e-2, src/model_operations.py:12) with r != 0.
Each file (below 1 MiB) holds
  dz                 seeded N(0,1) [R,5]
  grads, dX, dq0     float64 gradients rounded to float32 (parameters in blob order), read from .grad after .backward(): the
                     reference's re-entrant checkpoint refuses autograd.grad(inputs=...)
  E_ref              the tests' metric (training_fixture.grad_error) of the reference's own float32 parameter gradients
  E_ref_inputs       the same over {dX, dq0}
  n_fixup, dm        number of fix-up edges and the gradient that reaches max(D) through them (float64)
  D only: X, ids_topk, q_idx, res_of_atom
The script asserts that every gradient is finite, that the maximal edges are a single edge or the two directions of one pair, and that
A, C and D have fix-up edges with a non-zero gradient of max(D).

Usage:  python tests/golden/make_autograd_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch as pt

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import save  # noqa: E402
from make_training_golden import blob_of, build_model, metric, pesto_config  # noqa: E402


def load_case(name):
    g = np.load(os.path.join(OUT, f"training_{name}.npz"))
    X = pt.from_numpy(g["X"].astype(np.float32))
    ids = pt.from_numpy(g["ids_topk"].astype(np.int64))
    q = pt.zeros((X.shape[0], 30))
    q[pt.arange(X.shape[0]), pt.from_numpy(g["q_idx"].astype(np.int64))] = 1.0
    roa = g["res_of_atom"].astype(np.int64)
    M = pt.zeros((X.shape[0], int(roa.max()) + 1))
    M[pt.arange(X.shape[0]), pt.from_numpy(roa)] = 1.0
    return X, ids, q, M, g["sizes"]


def spy_max(store):
    """torch.max with a hook on the scalar maximum of unpack_state_features (:12): records the gradient that reaches it."""
    orig = pt.max

    def wrapped(*a, **k):
        out = orig(*a, **k)
        if isinstance(out, pt.Tensor) and out.ndim == 0 and out.requires_grad:
            out.register_hook(lambda g: store.append(float(g)))
        return out
    return orig, wrapped


def gradients(model, X, ids, q, M, dz, dtype, keys):
    m = copy.deepcopy(model).to(dtype)
    X = X.to(dtype).clone().requires_grad_()
    q = q.to(dtype).clone().requires_grad_()
    dm = []
    orig, wrapped = spy_max(dm)
    pt.max = wrapped
    try:
        z = m.forward(X, ids, q, M.to(dtype))
        pt.sum(z * pt.from_numpy(dz).to(dtype)).backward()
    finally:
        pt.max = orig
    return (blob_of(dict(m.named_parameters()), keys, "grad"), X.grad.double().numpy(), q.grad.double().numpy(), z.detach().numpy(),
            dm[0] if dm else 0.0)


def inputs_metric(dX, dq0, dX_ref, dq0_ref):
    """training_fixture.grad_error over the two input gradients: max over t of max|g - ref| / (max|ref_t| + 1e-3 max_all|ref|)"""
    floor = 1e-3 * max(np.abs(dX_ref).max(), np.abs(dq0_ref).max())
    return max(np.abs(dX - dX_ref).max() / (np.abs(dX_ref).max() + floor), np.abs(dq0 - dq0_ref).max() / (np.abs(dq0_ref).max() + floor))


def edge_facts(X, ids):
    """(number of fix-up edges, the maximal edges as (i, j) pairs) of the float32 geometry, src/model_operations.py:8-12"""
    R = X[ids - 1] - X.unsqueeze(1)
    D = pt.norm(R, dim=2)
    n_fix = int((D < 1e-2).sum())
    i, c = pt.nonzero(D == pt.max(D), as_tuple=True)
    j = (ids[i, c] - 1) % X.shape[0]
    return n_fix, sorted(set(zip(i.tolist(), j.tolist())))


def main():
    from pesto_amd.weights import blob_schema
    keys = blob_schema(pesto_config())
    model = build_model()      # (imports the reference: src.* is importable from here on)
    from src.data_encoding import extract_topology
    cases = {}
    for name in "ABC":
        cases[name] = load_case(name)
    X, ids, q, M, sizes = cases["B"]
    n = int(sizes[0])
    Xd = X[:n].clone()
    Xd[1] = Xd[0] + pt.tensor([3e-3, 4e-3, 0.0])      # 5e-3 A apart
    roa = M[:n].argmax(1)
    Md = pt.zeros((n, int(roa.max()) + 1))
    Md[pt.arange(n), roa] = 1.0
    cases["D"] = (Xd, extract_topology(Xd, 64)[0], q[:n].clone(), Md, np.array([n], np.int32))

    for seed, (name, (X, ids, q, M, sizes)) in enumerate(cases.items()):
        dz = np.random.default_rng(4100 + seed).standard_normal((M.shape[1], 5)).astype(np.float32)
        g32, dX32, dq32, z32, _ = gradients(model, X, ids, q, M, dz, pt.float32, keys)
        g64, dX64, dq64, z64, dm = gradients(model, X, ids, q, M, dz, pt.float64, keys)
        for a in (g32, dX32, dq32, g64, dX64, dq64):
            assert np.isfinite(a).all(), name
        n_fix, maximal = edge_facts(X, ids)
        assert len(maximal) == 1 or (len(maximal) == 2 and maximal[0] == maximal[1][::-1]), (name, maximal)
        if name in "ACD":
            assert n_fix > 0 and dm != 0.0, (name, n_fix, dm)
        e_ref, worst = metric(g32, g64, keys)
        e_in = inputs_metric(dX32, dq32, dX64, dq64)
        print(f"case {name}: N={X.shape[0]} R={M.shape[1]} fix-up edges={n_fix} d m={dm:.3e} maximal={maximal} max|dX|={np.abs(dX64).max():.3e} "
              f"max|dq0|={np.abs(dq64).max():.3e} E_ref={e_ref:.3e} ({worst}) E_ref_inputs={e_in:.3e} "
              f"dX32 err={np.abs(dX32 - dX64).max() / np.abs(dX64).max():.2e} dq32 err={np.abs(dq32 - dq64).max() / np.abs(dq64).max():.2e}")
        arrs = dict(dz=dz, grads=g64.astype(np.float32), dX=dX64.astype(np.float32), dq0=dq64.astype(np.float32), z=z32.astype(np.float32),
                    E_ref=np.float64(e_ref), E_ref_inputs=np.float64(e_in), n_fixup=np.int64(n_fix), dm=np.float64(dm))
        if name == "D":
            arrs.update(X=X.numpy(), ids_topk=ids.numpy().astype(np.int16), q_idx=q.numpy().argmax(1).astype(np.uint8),
                        res_of_atom=M.numpy().argmax(1).astype(np.int16), sizes=sizes)
        save("autograd_" + name, **arrs)


if __name__ == "__main__":
    main()
