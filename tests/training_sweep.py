"""Deterministic case generators of the training sweep (a plain module: tests/test_training_sweep_fixture.py checks the generators and the
definition without a GPU, tests/test_training_sweep.py puts every case through pesto_amd.training / pesto_amd.nn on one).

A case is a tuple (model, seed, shape). The lists below are fixed, so a failure names its case and two runs execute the same cases. Inputs
come from numpy.random.default_rng([seed, attempt]): a builder draws again (attempt 0, 1, ...) until the properties it promises hold.
They are properties of the inputs and of the definition (tests/model_def.py) alone; no builder looks at the library:
    every float64 gradient is finite and some parameter gradient is non-zero;
    no edge has D0 within 1e-6 relative of the 1e-2 fix-up threshold (float32 and float64 take the same decision);
    the maximal edge of the float32 geometry is unique or the two directions of one pair (k_unpack_bwd_max leaves other ties undefined);
    8 x E_ref < 1e-3, E_ref the metric of the definition's own float32 run against its float64 run: the cap of the bound never decides;
    a batch whose structures all have more than k + 1 atoms has no fix-up edge: nothing couples its structures (with k + 1 atoms an
    atom's own distance, moved to the maximum, ties with its farthest neighbour's and may stay in the list as an r = 0 edge).
The ids are pesto_amd.topology.extract_topology's (pinned by test_topology.py, not the code under test), collated into the Trainer's
convention: 1-based with the structure's offset, 0 = padding. Coordinates are uniform at 0.05 atoms / A^3, as the recorded cases'.

Models
    M4  training_fixture.CONFIG and state_dict(): layers 0 / 4 / 8 / 12 of the trained i_v4_0, n0 = 30, n_out = 5
    M3  the same four layers of the trained i_v3_0: n0 = 123, so the embed backward's feature loop runs 4 strides, the last one partial
    R1  make_config(1, [(8, 1)], n_out=1), seeded weights            R2  make_config(512, [(64, 1), (16, 1)], n_out=32), seeded weights
Seeded weights are drawn in blob_schema order, N(0, 1/fan_in) for matrices and N(0, 0.1^2) for biases; SEEDED_SHA256 holds the sha256
of the float32 blob, so a changed random stream is noticed instead of silently moving the yardstick.

Edges (pesto_train.hip): k_layer_v1_bwd<NN> gives one workgroup A = 64 / NN centres of the N + 1 state rows; k_head_sam_bwd and
k_embed_bwd take 8 atoms, k_head_decode_bwd 8 residues per workgroup; k_head_pool / k_head_pool_bwd walk one residue per wave with a
roa[i] == r filter; k_embed_bwd strides n0 by 32; dz / k_pos_ratios / k_loss take n_out <= 32; run_unpack takes k <= 64 id columns.
(N + 1) mod 8 = 1 needs N = 0 where N + 1 <= 8, so that regime asks for {0, 7} only.
"""
import functools
import hashlib

import numpy as np
import torch

from analysis_sweep import drawn, rows_of
from conftest import golden, onehot, weights
from model_def import Definition
from pesto_amd.config import make_config
from pesto_amd.topology import extract_topology
from pesto_amd.weights import blob_schema
from training_fixture import CONFIG, LAYERS, grad_error, state_dict

DTYPES = {32: torch.float32, 64: torch.float64}
SEEDED_SHA256 = {"R1": "ddee613df818ef6bcc679f259cbd80e903c54497b42d9355b9a68f2c53bf212e",
                 "R2": "3e8cdeb3be116febb4437647e7e7eed491f50508bb852fec5cb0e98bbd05f3a5"}
_models = {}


def case_id(case):
    model, seed, shape = case
    return f"{model}_s{seed}_" + "x".join("-".join(str(a) for a in v) if isinstance(v, tuple) else str(v) for v in shape)


# ================================================================== models
def seeded_state(cfg, seed):
    rng = np.random.default_rng(seed)
    sd = {}
    for key, shape in blob_schema(cfg):
        sd[key] = ((rng.standard_normal(shape) / np.sqrt(shape[1])) if len(shape) == 2 else 0.1 * rng.standard_normal(shape)).astype(np.float32)
    return sd


def blob_sha256(cfg, sd):
    return hashlib.sha256(np.concatenate([np.ascontiguousarray(sd[k], np.float32).ravel() for k, _ in blob_schema(cfg)]).tobytes()).hexdigest()


def model(name):
    """(config, state_dict of numpy arrays)"""
    if name not in _models:
        if name == "M4":
            _models[name] = (CONFIG, state_dict())
        elif name == "M3":
            sd = {}
            for k, v in weights("i_v3_0").items():
                if k.startswith("sum."):
                    parts = k.split(".")
                    if int(parts[1]) not in LAYERS:
                        continue
                    k = ".".join(["sum", str(LAYERS.index(int(parts[1])))] + parts[2:])
                sd[k] = v
            _models[name] = (make_config(123, [(8, 1), (16, 1), (32, 1), (64, 1)]), sd)
        elif name == "R1":
            cfg = make_config(1, [(8, 1)], n_out=1)
            _models[name] = (cfg, seeded_state(cfg, 9101))
        elif name == "R2":
            cfg = make_config(512, [(64, 1), (16, 1)], n_out=32)
            _models[name] = (cfg, seeded_state(cfg, 9102))
        else:
            raise KeyError(name)
    return _models[name]


def keys(name, prefixes=None):
    return [(k, s) for k, s in blob_schema(model(name)[0]) if prefixes is None or k.startswith(prefixes)]


@functools.lru_cache(maxsize=None)
def definition(name, bits):
    cfg, sd = model(name)
    return Definition(cfg, {k: sd[k] for k, _ in blob_schema(cfg)}, DTYPES[bits])


# ================================================================== the definition's gradients (any Definition: the fixture test calls
# these on the recorded inputs too)
def step_def(d, X, ids, q0, roa, R, y, global_step):
    """loss_and_grad: z, p, losses, pos_ratios and the parameter gradients of sum(losses)"""
    d.zero_grad()
    z = d.forward(X, ids, q0, roa, R)
    losses, pos = d.loss(z, y, global_step)
    losses.sum().backward()
    out = dict(z=z, p=torch.sigmoid(z), losses=losses, pos=pos)
    return dict({k: v.detach().double().numpy() for k, v in out.items()}, grads=d.grads())


def autograd_def(d, X, ids, q0, roa, R, dz):
    """the gradients of sum(z * dz): parameters, dX, dq0; n_fixup and the gradient that reaches max D0"""
    d.zero_grad()
    X = d.t(X).requires_grad_()
    q0 = d.t(q0).requires_grad_()
    z = d.forward(X, ids, q0, roa, R)
    (z * d.t(dz)).sum().backward()
    return dict(z=z.detach().double().numpy(), grads=d.grads(), dX=X.grad.double().numpy(), dq0=q0.grad.double().numpy(),
                n_fixup=int((d.D0 < 1e-2).sum()), dm=0.0 if d.dmax.grad is None else float(d.dmax.grad))


def layer_def(d, l, X, ids, q_in, p_in, dq_out, dp_out):
    d.zero_grad()
    q = d.t(q_in).requires_grad_()
    p = d.t(p_in).requires_grad_()
    with torch.no_grad():
        ids_s, D, R = d.unpack(X, ids)
    q2, p2 = d.layer(l, q, p, ids_s, D, R)
    ((q2 * d.t(dq_out)).sum() + (p2 * d.t(dp_out)).sum()).backward()
    return dict(dq_in=q.grad.double().numpy(), dp_in=p.grad.double().numpy(), grads=d.grads(f"sum.{l}."))


def head_def(d, q, p, roa, R, dz):
    d.zero_grad()
    q = d.t(q).requires_grad_()
    p = d.t(p).requires_grad_()
    (d.head(q, p, roa, R) * d.t(dz)).sum().backward()
    return dict(dq=q.grad.double().numpy(), dp=p.grad.double().numpy(), grads=d.grads(("spl.", "dm.")))


def embed_def(d, q0, dq):
    d.zero_grad()
    (d.embed(q0) * d.t(dq)).sum().backward()
    return dict(grads=d.grads("em."))


def worst(err):
    k = max(err, key=err.get)
    return err[k], k


# ================================================================== bounds
@functools.lru_cache(maxsize=None)
def e_floor(kind):
    """the smallest float32-vs-float64 error the committed fixtures record for that kind of gradient"""
    return float(golden("autograd_B")["E_ref" if kind == "parameters" else "E_ref_inputs"])


def bound(kind, e_ref):
    """training_fixture.grad_bound with the floor: min(1e-3, 8 x max(E_ref(case), E_floor))"""
    return min(1e-3, 8.0 * max(float(e_ref), e_floor(kind)))


# ================================================================== inputs
def cloud(rng, n):
    side = (n / 0.05) ** (1.0 / 3.0)
    return rng.uniform(0.0, side, (n, 3)).astype(np.float32)


def collate(Xs, k):
    """ids [N,k] int32 in the Trainer's convention from the structures' own topologies"""
    N = sum(x.shape[0] for x in Xs)
    ids = np.zeros((N, k), np.int32)
    off = 0
    for x in Xs:
        t = np.asarray(extract_topology(x, k)).astype(np.int32)
        ids[off:off + x.shape[0], :t.shape[1]] = t + off + 1
        off += x.shape[0]
    return np.concatenate(Xs, 0), ids


def residues(rng, sizes, layout):
    out, off = [], 0
    for n in sizes:
        r = np.arange(n, dtype=np.int32) // 8 if layout == "eights" else rows_of(rng, n, layout)
        out.append(r + off)
        off += int(r.max()) + 1
    return np.concatenate(out).astype(np.int32), off


def features(rng, name, N):
    n0 = model(name)[0]["em"]["N0"]
    if name == "M4":
        return onehot(rng.integers(0, 30, (N, 1)), 30)
    if name == "M3":
        return onehot(np.stack([rng.integers(0, 30, N), rng.integers(0, 29, N), rng.integers(0, 64, N)], 1), 123)
    return rng.standard_normal((N, n0)).astype(np.float32)


def geometry_facts(X, ids):
    """of the float32 geometry: (the edges keep clear of the fix-up threshold, the maximal edges as (i, j) pairs)"""
    N = X.shape[0]
    j = (ids.astype(np.int64) - 1) % N
    r = X[j] - X[:, None, :]
    D = np.sqrt((r * r).sum(-1, dtype=np.float32))
    D64 = np.sqrt((r.astype(np.float64) ** 2).sum(-1))
    clear = bool((np.abs(D64 - 1e-2) > 1e-8).all())
    i, c = np.nonzero(D == D.max())
    return clear, sorted(set(zip(i.tolist(), j[i, c].tolist())))


def geometry_ok(X, ids):
    clear, maximal = geometry_facts(X, ids)
    return clear and (len(maximal) == 1 or (len(maximal) == 2 and maximal[0] == maximal[1][::-1]))


def redrawn(draw, case, tries=40):
    """analysis_sweep.drawn over a draw that returns the case or the promise it misses (a string, kept for the failure's message)"""
    missed = []

    def attempt(rng):
        c = draw(rng)
        if isinstance(c, str):
            missed.append(c)
            return None
        return c
    try:
        return drawn(attempt, case[1], tries)
    except AssertionError as err:
        raise AssertionError(f"{case_id(case)}: {err}; first misses: {missed[:3]}") from None


def finite(*dicts):
    return all(np.isfinite(v).all() for d in dicts for v in d.values())


# ================================================================== whole-step cases: shape (sizes, layout, k, ids as, y, global_step)
# (with R = 1 a column of y is all zero or all one, and at global_step 0 the loss is then zero or 0 / 0: those cases run at step 1)
# y: "rand" Bernoulli(0.3); "zero" / "one": its first / last column all zero / all one
STEP = (
    ("M4", 101, ((2,), "one", 64, "i32", "rand", 0)),
    ("M4", 102, ((6,), "all", 64, "i64", "rand", 1)),
    ("M4", 103, ((7,), "one", 64, "i32", "zero", 0)),
    ("M4", 104, ((8,), "one", 64, "i64", "one", 0)),
    ("M4", 105, ((9,), "one", 64, "i32", "rand", 1)),
    ("M4", 106, ((15,), "mixed", 64, "i64", "rand", 0)),
    ("M4", 107, ((16,), "eights", 64, "i32", "rand", 0)),
    ("M4", 108, ((17,), "one", 64, "i32", "rand", 0)),
    ("M4", 109, ((63,), "mixed", 64, "i64", "zero", 1)),
    ("M4", 110, ((64,), "all", 64, "i32", "rand", 1)),
    ("M4", 111, ((65,), "all", 64, "i32", "rand", 1)),
    ("M4", 112, ((129,), "all", 64, "i64", "rand", 1)),
    ("M4", 113, ((6, 8), "eights", 64, "i32", "rand", 0)),
    ("M4", 114, ((66, 70), "mixed", 64, "i64", "rand", 0)),
    ("M4", 115, ((9, 2, 17), "eights", 64, "i32", "one", 0)),
    ("M3", 121, ((8,), "eights", 64, "i32", "rand", 1)),
    ("M3", 122, ((17,), "mixed", 64, "i64", "rand", 0)),
    ("M3", 123, ((65,), "eights", 64, "i32", "rand", 1)),
    ("M3", 124, ((7, 9), "one", 64, "i64", "zero", 0)),
    ("R1", 131, ((9,), "one", 8, "i64", "rand", 0)),
    ("R1", 132, ((16,), "eights", 16, "i32", "rand", 1)),
    ("R1", 133, ((6,), "all", 8, "i32", "rand", 1)),
    ("R1", 134, ((64,), "mixed", 64, "i64", "rand", 0)),
    ("R2", 141, ((7,), "one", 64, "i32", "rand", 0)),
    ("R2", 142, ((17,), "mixed", 64, "i64", "one", 0)),
    ("R2", 143, ((65,), "all", 64, "i32", "rand", 1)),
    ("R2", 144, ((56,), "eights", 64, "i64", "zero", 0)),
)
INDEPENDENT = STEP[13]      # every structure above 64 + 1 atoms: the case of the independence check


def build_step(case):
    name, seed, (sizes, layout, k, ids_as, ymode, step) = case
    C = model(name)[0]["dm"]["N2"]
    d64, d32 = definition(name, 64), definition(name, 32)

    def draw(rng):
        X, ids = collate([cloud(rng, n) for n in sizes], k)
        N = X.shape[0]
        roa, R = residues(rng, sizes, layout)
        q0 = features(rng, name, N)
        y = (rng.random((R, C)) < 0.3).astype(np.float32)
        if ymode == "zero":
            y[:, 0] = 0.0
        if ymode == "one":
            y[:, C - 1] = 1.0
        dz = rng.standard_normal((R, C)).astype(np.float32)
        if not geometry_ok(X, ids):
            return "geometry"
        batch = (X, ids, q0, roa, R)
        s64, a64 = step_def(d64, *batch, y, step), autograd_def(d64, *batch, dz)
        if not (finite(s64["grads"], a64["grads"], dict(dX=a64["dX"], dq0=a64["dq0"], l=s64["losses"]))
                and max(np.abs(v).max() for v in s64["grads"].values()) > 0):
            return "a gradient is not finite, or all are zero"
        if min(sizes) > k + 1 and a64["n_fixup"]:
            return "fix-up edges"
        s32, a32 = step_def(d32, *batch, y, step), autograd_def(d32, *batch, dz)
        inputs = lambda a: dict(dX=a["dX"], dq0=a["dq0"])      # noqa: E731
        e = dict(step=worst(grad_error(s32["grads"], s64["grads"])), parameters=worst(grad_error(a32["grads"], a64["grads"])),
                 inputs=worst(grad_error(inputs(a32), inputs(a64))))
        if not all(8.0 * v[0] < 1e-3 for v in e.values()):
            return f"E_ref {e}"
        return dict(X=X, ids=ids, q0=q0, roa=roa, R=R, y=y, dz=dz, step=step, ids_as=ids_as, sizes=sizes, s64=s64, a64=a64, e_ref=e)
    return redrawn(draw, case)


# ================================================================== stage cases
# layer: shape (layer of M4, N); the N + 1 state rows are what the workgroups split. (N + 1 = 2 is N = 1, whose only edge has length 0 and
# a fix-up of 0: the definition divides by zero there as in a whole step, so nn = 32 runs N + 1 = 3, 4 and 9)
LAYER = tuple(("M4", 200 + i, (l, n1 - 1)) for i, (l, n1) in enumerate(
    [(0, 7), (0, 8), (0, 9), (0, 16), (0, 17), (1, 4), (1, 5), (1, 8), (1, 9), (2, 3), (2, 4), (2, 9), (3, 3), (3, 65), (3, 66)]))
# head: shape (N, layout)
HEAD_SHAPES = ((7, "one"), (8, "one"), (9, "one"), (17, "one"), (16, "eights"), (63, "mixed"), (64, "all"), (65, "all"), (129, "all"))
HEAD = tuple((m, 300 + 20 * j + i, s) for j, m in enumerate(("M4", "R2")) for i, s in enumerate(HEAD_SHAPES))
# embed: shape (N,)
EMBED = tuple((m, 400 + 10 * j + i, (n,)) for j, m in enumerate(("M3", "R2")) for i, n in enumerate((7, 8, 9, 17)))


def build_layer(case):
    name, seed, (l, N) = case
    d64, d32 = definition(name, 64), definition(name, 32)

    def draw(rng):
        X, ids = collate([cloud(rng, N)], 64)
        normal = lambda *s: rng.standard_normal(s).astype(np.float32)      # noqa: E731
        q_in, p_in, dq_out, dp_out = normal(N + 1, 32), normal(N + 1, 3, 32), normal(N + 1, 32), normal(N + 1, 3, 32)
        q_in[0] = 0.0      # the sink row of a state is zero
        p_in[0] = 0.0
        if not geometry_facts(X, ids)[0]:
            return "geometry"
        args = (l, X, ids, q_in, p_in, dq_out, dp_out)
        r64, r32 = layer_def(d64, *args), layer_def(d32, *args)
        states = lambda r: dict(dq_in=r["dq_in"][1:], dp_in=r["dp_in"][1:])      # noqa: E731
        e = dict(parameters=worst(grad_error(r32["grads"], r64["grads"])), inputs=worst(grad_error(states(r32), states(r64))))
        if not (finite(r64["grads"], states(r64)) and all(8.0 * v[0] < 1e-3 for v in e.values())):
            return f"E_ref {e}"
        return dict(args=args, r64=r64, e_ref=e)
    return redrawn(draw, case)


def build_head(case):
    name, seed, (N, layout) = case
    C = model(name)[0]["dm"]["N2"]
    d64, d32 = definition(name, 64), definition(name, 32)

    def draw(rng):
        roa, R = residues(rng, (N,), layout)
        args = (rng.standard_normal((N, 32)).astype(np.float32), rng.standard_normal((N, 3, 32)).astype(np.float32), roa, R,
                rng.standard_normal((R, C)).astype(np.float32))
        r64, r32 = head_def(d64, *args), head_def(d32, *args)
        states = lambda r: dict(dq=r["dq"], dp=r["dp"])      # noqa: E731
        e = dict(parameters=worst(grad_error(r32["grads"], r64["grads"])), inputs=worst(grad_error(states(r32), states(r64))))
        if not (finite(r64["grads"], states(r64)) and all(8.0 * v[0] < 1e-3 for v in e.values())):
            return f"E_ref {e}"
        return dict(args=args, r64=r64, e_ref=e)
    return redrawn(draw, case)


def build_embed(case):
    name, seed, (N,) = case
    d64, d32 = definition(name, 64), definition(name, 32)

    def draw(rng):
        args = (features(rng, name, N), rng.standard_normal((N, 32)).astype(np.float32))
        r64, r32 = embed_def(d64, *args), embed_def(d32, *args)
        e = dict(parameters=worst(grad_error(r32["grads"], r64["grads"])))
        if not (finite(r64["grads"]) and 8.0 * e["parameters"][0] < 1e-3):
            return f"E_ref {e}"
        return dict(args=args, r64=r64, e_ref=e)
    return redrawn(draw, case)


# ================================================================== the registry
CASES = dict(step=STEP, layer=LAYER, head=HEAD, embed=EMBED)
BUILDERS = dict(step=build_step, layer=build_layer, head=build_head, embed=build_embed)


@functools.lru_cache(maxsize=None)
def build(entry, case):
    """the case's inputs, the definition's float64 results and E_ref - computed once, shared by the tests and left unchanged"""
    return BUILDERS[entry](case)


def all_cases():
    return [(entry, case) for entry, cases in CASES.items() for case in cases]


def every_third(entry, case):
    """the cases that also run from ROCm tensors"""
    return CASES[entry].index(case) % 3 == 0


def layout_facts(sizes, layout, seed):
    """(R, the largest residue's atoms, whether two residues' atoms interleave) of a case's residue map - attempt 0's, whose R and sizes
    every attempt of 'eights', 'one' and 'all' shares"""
    roa, R = residues(np.random.default_rng([seed, 0]), sizes, layout)
    first = {r: int(np.nonzero(roa == r)[0][0]) for r in range(R)}
    last = {r: int(np.nonzero(roa == r)[0][-1]) for r in range(R)}
    interleaved = any(last[r] - first[r] + 1 > int((roa == r).sum()) for r in range(R))
    return R, int(np.bincount(roa).max()), interleaved


def coverage():
    """{(case list, edge): the set of values the list's shapes hit}"""
    t = {}

    def hit(entry, name, values):
        t.setdefault((entry, name), set()).update(values)
    for name, seed, (sizes, layout, k, ids_as, ymode, step) in STEP:
        cfg = model(name)[0]
        N = sum(sizes)
        hit("step", "(N+1)%8, N+1>8" if N + 1 > 8 else "(N+1)%8, N+1<=8", [(N + 1) % 8])
        hit("step", "(N+1)%4", [(N + 1) % 4]); hit("step", "(N+1)%2", [(N + 1) % 2]); hit("step", "N", [N]); hit("step", "N%8", [N % 8])
        R, largest, _ = layout_facts(sizes, layout, seed)
        if layout != "mixed":      # (a mixed layout's R and sizes are the draw's)
            hit("step", "R", [R]); hit("step", "largest residue", [largest])
        hit("step", "layout", [layout]); hit("step", "structures", [len(sizes)])
        hit("step", "batch", ["all>64"] * (min(sizes) > 64) + ["one<8"] * (min(sizes) < 8))
        hit("step", "n0", [cfg["em"]["N0"]]); hit("step", "n_out", [cfg["dm"]["N2"]]); hit("step", "k", [(k, name) if k == 16 else k])
        hit("step", "ids", [ids_as]); hit("step", "y", [ymode]); hit("step", "global_step", [step])
    for _, _, (l, N) in LAYER:
        hit("layer", f"nn={CONFIG['sum'][l]['nn']}:N+1", [N + 1])
    for name, seed, (N, layout) in HEAD:
        R, largest, _ = layout_facts((N,), layout, seed)
        if layout != "mixed":
            hit("head", f"{name}:R", [R]); hit("head", f"{name}:largest residue", [largest])
        hit("head", f"{name}:layout", [layout])
    for name, _, (N,) in EMBED:
        hit("embed", f"{name}:N%8", [N % 8])
    return t


REQUIRED = {
    ("step", "(N+1)%8, N+1>8"): {0, 1, 7}, ("step", "(N+1)%8, N+1<=8"): {0, 7}, ("step", "(N+1)%4"): {0, 1, 3}, ("step", "(N+1)%2"): {0, 1},
    ("step", "N"): {2, 6, 7, 8, 9, 15, 16, 17, 63, 64, 65, 129}, ("step", "N%8"): {0, 1, 7}, ("step", "R"): {1, 7, 8, 9, 17},
    ("step", "largest residue"): {1, 8, 64, 65, 129}, ("step", "layout"): {"eights", "one", "all", "mixed"}, ("step", "structures"): {1, 2, 3},
    ("step", "batch"): {"all>64", "one<8"}, ("step", "n0"): {1, 30, 123, 512}, ("step", "n_out"): {1, 5, 32}, ("step", "k"): {8, (16, "R1"), 64},
    ("step", "ids"): {"i32", "i64"}, ("step", "y"): {"rand", "zero", "one"}, ("step", "global_step"): {0, 1},
    ("layer", "nn=8:N+1"): {7, 8, 9, 16, 17}, ("layer", "nn=16:N+1"): {4, 5, 8, 9}, ("layer", "nn=32:N+1"): {3, 4, 9}, ("layer", "nn=64:N+1"): {3, 65, 66},
    ("head", "M4:R"): {1, 7, 8, 9, 17}, ("head", "R2:R"): {1, 7, 8, 9, 17}, ("head", "M4:largest residue"): {1, 8, 64, 65, 129},
    ("head", "R2:largest residue"): {1, 8, 64, 65, 129}, ("head", "M4:layout"): {"eights", "one", "all", "mixed"},
    ("head", "R2:layout"): {"eights", "one", "all", "mixed"}, ("embed", "M3:N%8"): {0, 1, 7}, ("embed", "R2:N%8"): {0, 1, 7},
}
