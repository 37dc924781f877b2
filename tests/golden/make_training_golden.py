#!/usr/bin/env python3
"""Generate tests/golden/training*.npz: the reference's training step (model/main.py:42-58, 186-200) on its PyTorch CPU path, in
float32 and in float64, for pesto_amd.training. The reference is IMPORTED (make_golden.import_reference, with the gemmi stub); what is
committed is data plus this script.

Model: the trained i_v4_0 checkpoint, layers 0, 4, 8 and 12 renumbered 0..3 (nn = 8, 16, 32, 64).
Inputs: seeded uniform clouds at density 0.05 / A^3, residues of 8 consecutive atoms, y ~ Bernoulli(0.2), one column of case B all zero.
  A  N = 40                 fewer than 64 atoms: zero-padded slots and the wrap
  B  N = 200 + 70 collated  id offsets, R normalisation, N + 1 = 271
  C  N = 64 + 65 + 8        k exactly N, a one-atom residue, a one-residue structure
Files (each below 1 MiB):
  training_{A,B,C}.npz      inputs, z / losses / pos_ratios (float32 run, global_step 0), float64 gradients rounded to float32 in blob
                            order, E_ref = the tests' metric applied to the reference's own float32 gradients
  training_stage_L{0..3}.npz, training_stage_head.npz
                            stage backward on case B's float32 states, evaluated in float64: seeded output gradients, the
                            reference's input and weight gradients (layers; pool + dm; embed)
  training_curve.npz        24 Adam steps at lr = 1e-3 on B's first structure: float64 loss curve and the reference's own
                            float32-vs-float64 deviation

Usage:  python tests/golden/make_training_golden.py
"""
import copy
import os
import sys

import numpy as np
import torch as pt

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, OUT)
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))
from make_golden import collate, import_reference, save  # noqa: E402

RUN = "i_v4_0_2021-09-07_11-20"
LAYERS = (0, 4, 8, 12)
POS_WEIGHT_FACTOR = 0.5


def pesto_config():
    from pesto_amd.config import make_config
    return make_config(30, [(8, 1), (16, 1), (32, 1), (64, 1)])


def build_model():
    cfg, Model, save_path = import_reference(RUN)
    cfg4 = copy.deepcopy(cfg)
    cfg4["sum"] = [cfg["sum"][i] for i in LAYERS]
    sd = pt.load(os.path.join(save_path, "model_ckpt.pt"), map_location="cpu")
    sd4 = {}
    for k, v in sd.items():
        if k.startswith("sum."):
            parts = k.split(".")
            if int(parts[1]) not in LAYERS:
                continue
            k = ".".join(["sum", str(LAYERS.index(int(parts[1])))] + parts[2:])
        sd4[k] = v
    model = Model(cfg4)
    print(model.load_state_dict(sd4))
    return model


def structure(n, rng):
    from src.data_encoding import extract_topology
    side = (n / 0.05) ** (1.0 / 3.0)
    X = pt.from_numpy(rng.uniform(0.0, side, (n, 3)).astype(np.float32))
    ids = extract_topology(X, 64)[0]
    q = np.zeros((n, 30), np.float32)
    q[np.arange(n), rng.integers(0, 30, n)] = 1.0
    R = (n + 7) // 8
    M = np.zeros((n, R), np.float32)
    M[np.arange(n), np.arange(n) // 8] = 1.0
    return [X, ids, pt.from_numpy(q), pt.from_numpy(M)]


def eval_step(model, batch, pos_ratios, global_step):
    """model/main.py:42-58 (pos_ratios is updated in place, as there)"""
    X, ids, q, M, y = batch
    z = model.forward(X, ids, q, M)
    pos_ratios += (pt.mean(y, dim=0).detach() - pos_ratios) / (1.0 + np.sqrt(global_step))
    criterion = pt.nn.BCEWithLogitsLoss(reduction="none")
    criterion.pos_weight = POS_WEIGHT_FACTOR * (1.0 - pos_ratios) / (pos_ratios + 1e-6)
    dloss = criterion(z, y)
    losses = ((pos_ratios / pt.sum(pos_ratios)).reshape(1, -1) * dloss) / dloss.shape[0]
    return losses, z


def cast(batch, dtype):
    return [t.to(dtype) if t.is_floating_point() else t for t in batch]


def blob_of(named, keys, attr=None):
    parts = []
    for k, shape in keys:
        t = named[k] if attr is None else getattr(named[k], attr)
        assert tuple(t.shape) == tuple(shape), k
        parts.append(t.detach().double().numpy().ravel())
    return np.concatenate(parts)


def metric(g, ref, keys):
    """max over tensors t of max|g - ref| / (max|ref_t| + 1e-3 max_all|ref|); returns (E, worst key)"""
    floor = 1e-3 * np.abs(ref).max()
    off, worst = 0, (0.0, None)
    for k, shape in keys:
        n = int(np.prod(shape))
        e = np.abs(g[off:off + n] - ref[off:off + n]).max() / (np.abs(ref[off:off + n]).max() + floor)
        if e > worst[0]:
            worst = (e, k)
        off += n
    return worst


def loss_and_grad(model, batch, dtype, global_step, keys):
    model = copy.deepcopy(model).to(dtype)
    pos = 0.5 * pt.ones(batch[4].shape[1], dtype=dtype)
    losses, z = eval_step(model, cast(batch, dtype), pos, global_step)
    pt.sum(losses).backward()
    return losses.detach().numpy(), z.detach().numpy(), pos.numpy(), blob_of(dict(model.named_parameters()), keys, "grad")


def idx_of(q):
    return q.numpy().argmax(1).astype(np.uint8)


def roa_of(M):
    return M.numpy().argmax(1).astype(np.int16)


def main():
    from pesto_amd.weights import blob_schema
    keys = blob_schema(pesto_config())
    model = build_model()
    rng = np.random.default_rng(2024)
    cases = {"A": [40], "B": [200, 70], "C": [64, 65, 8]}
    batches = {}
    for name, sizes in cases.items():
        items = [structure(n, rng) for n in sizes]
        X, ids, q, M = collate(items)
        y = (rng.random((M.shape[1], 5)) < 0.2).astype(np.float32)
        if name == "B":
            y[:, 2] = 0.0
        batch = [X, ids, q, M, pt.from_numpy(y)]
        batches[name] = (batch, items)
        l32, z32, pos32, g32 = loss_and_grad(model, batch, pt.float32, 0, keys)
        l64, z64, pos64, g64 = loss_and_grad(model, batch, pt.float64, 0, keys)
        l32s1, _, pos32s1, _ = loss_and_grad(model, batch, pt.float32, 1, keys)
        e_ref, worst = metric(g32, g64, keys)
        print(f"case {name}: N={X.shape[0]} R={M.shape[1]} loss={l64.sum():.6f} E_ref={e_ref:.3e} ({worst}) |z32-z64|={np.abs(z32 - z64).max():.2e} "
              f"|l32-l64|={np.abs(l32 - l64).max():.2e}")
        save("training_" + name, X=X.numpy(), ids_topk=ids.numpy().astype(np.int16), q_idx=idx_of(q), res_of_atom=roa_of(M), y=y.astype(np.uint8),
             sizes=np.array(sizes, np.int32), z=z32.astype(np.float32), losses=l32.astype(np.float32), pos_ratios=pos32.astype(np.float32),
             losses_step1=l32s1.astype(np.float32), pos_ratios_step1=pos32s1.astype(np.float32),
             grads=g64.astype(np.float32), E_ref=np.float64(e_ref))

    # ------------------------------------------------------------------ stage backward on case B's float32 states, in float64
    from src.model_operations import unpack_state_features
    (X, ids, q0, M, y), items = batches["B"]
    m64 = copy.deepcopy(model).double()
    with pt.no_grad():
        q1 = model.em(q0)
        qs, ids_s, D, R = unpack_state_features(X, ids, q1)
        states = [(qs, pt.zeros((qs.shape[0], 3, qs.shape[1])))]
        for layer in model.sum:
            out = layer((states[-1][0].clone(), states[-1][1].clone(), ids_s, D, R))
            states.append((out[0].detach(), out[1].detach()))
        _, _, D64, R64 = unpack_state_features(X.double(), ids, q1.double())
    srng = np.random.default_rng(77)

    def named_grads(module, prefix):
        return {prefix + k: p for k, p in module.named_parameters() if p.requires_grad}

    for li, layer in enumerate(m64.sum):
        m64.zero_grad()
        q = states[li][0].double().requires_grad_()
        p = states[li][1].double().requires_grad_()
        dq = srng.standard_normal(tuple(q.shape)).astype(np.float32)
        dp = srng.standard_normal(tuple(p.shape)).astype(np.float32)
        out = layer((q, p, ids_s, D64, R64))
        (pt.sum(out[0] * pt.from_numpy(dq).double()) + pt.sum(out[1] * pt.from_numpy(dp).double())).backward()
        lk = [(k, s) for k, s in keys if k.startswith(f"sum.{li}.")]
        gw = blob_of(named_grads(layer, f"sum.{li}."), lk, "grad")
        print(f"stage L{li}: |dq_in|max={q.grad.abs().max():.3e} |dp_in|max={p.grad.abs().max():.3e} |gw|max={np.abs(gw).max():.3e}")
        save(f"training_stage_L{li}", q_in=states[li][0].numpy(), p_in=states[li][1].numpy(), dq_out=dq, dp_out=dp,
             dq_in=q.grad.numpy().astype(np.float32), dp_in=p.grad.numpy().astype(np.float32), grads=gw.astype(np.float32))
    # pool + dm
    m64.zero_grad()
    q = states[-1][0][1:].double().requires_grad_()
    p = states[-1][1][1:].double().requires_grad_()
    dz = srng.standard_normal((M.shape[1], 5)).astype(np.float32)
    qr, pr = m64.spl(q, p, M.double())
    z = m64.dm(pt.cat([qr, pt.norm(pr, dim=1)], dim=1))
    pt.sum(z * pt.from_numpy(dz).double()).backward()
    hk = [(k, s) for k, s in keys if k.startswith(("spl.", "dm."))]
    named = named_grads(m64.spl, "spl.")
    named.update(named_grads(m64.dm, "dm."))
    g_head = blob_of(named, hk, "grad")
    head = dict(q=states[-1][0][1:].numpy(), p=states[-1][1][1:].numpy(), dz=dz, dq=q.grad.numpy().astype(np.float32),
                dp=p.grad.numpy().astype(np.float32), grads_head=g_head.astype(np.float32))
    # embed
    m64.zero_grad()
    dq1 = srng.standard_normal((q0.shape[0], 32)).astype(np.float32)
    pt.sum(m64.em(q0.double()) * pt.from_numpy(dq1).double()).backward()
    ek = [(k, s) for k, s in keys if k.startswith("em.")]
    head.update(dq_em=dq1, grads_em=blob_of(named_grads(m64.em, "em."), ek, "grad").astype(np.float32))
    save("training_stage_head", **head)

    # ------------------------------------------------------------------ loss curve: 24 Adam steps at lr = 1e-3 on B's first structure
    Xc, idsc, qc, Mc = collate([items[0]])
    yc = pt.from_numpy((np.random.default_rng(5).random((Mc.shape[1], 5)) < 0.2).astype(np.float32))
    curves = {}
    for dtype in (pt.float32, pt.float64):
        m = copy.deepcopy(model).to(dtype)
        opt = pt.optim.Adam(m.parameters(), lr=1e-3)
        pos = 0.5 * pt.ones(5, dtype=dtype)
        batch = cast([Xc, idsc, qc, Mc, yc], dtype)
        curve = []
        for step in range(1, 25):
            opt.zero_grad()
            losses, _ = eval_step(m, batch, pos, step)
            loss = pt.sum(losses)
            loss.backward()
            opt.step()
            curve.append(float(loss))
        curves[dtype] = np.array(curve)
    dev = np.abs(curves[pt.float32] - curves[pt.float64]).max()
    print("curve64", np.round(curves[pt.float64], 4), "float32-vs-float64 deviation", dev)
    save("training_curve", X=Xc.numpy(), ids_topk=idsc.numpy().astype(np.int16), q_idx=idx_of(qc), res_of_atom=roa_of(Mc), y=yc.numpy().astype(np.uint8),
         loss64=curves[pt.float64], deviation=np.float64(dev))


if __name__ == "__main__":
    main()
