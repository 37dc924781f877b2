"""The reference's training step (model/main.py:42-58, 186-200) on the MI355X: forward, loss, backward and Adam in libpesto_hip.so.

    from pesto_amd.training import Trainer, scoring
    tr = Trainer(config, state_dict, device=0, lr=1e-5, pos_weight_factor=0.5)      # pos_ratios = 0.5, global_step = 0 (main.py:134-136)
    losses, y, p = tr.eval_step(X, ids_topk, q, M, y)             # main.py:42-58 without gradient (the test phase, :225-233)
    losses, p, grads = tr.loss_and_grad(X, ids_topk, q, M, y)     # grads: {state_dict key: float32 array}; no update
    losses, y, p = tr.train_step(X, ids_topk, q, M, y)            # main.py:186-200: global_step += 1, forward, loss, backward, Adam
    tr.state_dict(); tr.pos_ratios; tr.global_step; tr.model()
    scores = scoring(eval_results)                                # main.py:61-79 over evaluate.bc_scoring

Everything is float32. The forward is the exact fp32 layer kernel (no f16 split, no ``auto`` policy) and keeps the input state of every
layer; the backward recomputes each layer from it, like the reference's ``checkpoint`` (src/model_operations.py:234-236). One call takes
one collated batch with ``Model.forward``'s semantics. ``pos_ratios`` lives on the device and is updated there by every one of the three
calls, as ``eval_step`` does in the reference. Inputs are numpy arrays, CPU tensors or ROCm tensors (X decides where the call runs,
pesto_amd._lib.Side); ``M`` is the dense mask [N, R] or a pair ``(res_of_atom, R)``.

Sums that several workgroups contribute to (weight gradients, the gather's scatter-add) use 64-bit fixed-point atomics with 40 fractional
bits instead of float atomics: the result does not depend on the order in which the workgroups arrive, so a step is bit-reproducible
from run to run. The price is a fixed range: single terms are clamped to +-4e6 and a sum wraps beyond +-8.4e6.
There is no CPU or PyTorch fallback: without a GPU the constructor raises PestoError.
"""
import ctypes

import numpy as np

from . import _lib
from .config import normalise
from .topology import mask_to_segments
from .weights import blob_schema, flatten_state_dict, unflatten_blob

MODE_EVAL, MODE_GRAD, MODE_TRAIN = 0, 1, 2


def _check(rc):
    _lib.check(rc, _lib.load().pesto_train_last_error)


class Trainer:
    def __init__(self, config, state_dict, device=0, lr=1e-5, pos_weight_factor=0.5):
        self.config = normalise(config)
        if self.config["em_depth"] != 3 or self.config["dm_depth"] != 3:
            raise ValueError("training needs the three-Linear em and dm (em_depth = dm_depth = 3)")
        self._keys = blob_schema(self.config)
        self._gpu = int(device)
        self._handle = None
        self.last_z = None
        blob = np.ascontiguousarray(flatten_state_dict(self.config, state_dict), dtype=np.float32)
        self._n = int(blob.size)
        self._cc = _lib.make_c_config(self.config, "fp32")
        h = ctypes.c_void_p()
        _check(_lib.load().pesto_train_create(ctypes.byref(self._cc), blob.ctypes.data, blob.size, self._gpu, float(lr), float(pos_weight_factor),
                                              ctypes.byref(h)))
        self._handle = h

    def close(self):
        if self._handle is not None:
            _lib.load().pesto_train_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ------------------------------------------------------------------ state
    def _get(self, weights=False, pos=False):
        w = np.empty(self._n, np.float32) if weights else None
        pr = np.empty(self.config["dm"]["N2"], np.float32) if pos else None
        step, lr = ctypes.c_int64(), ctypes.c_float()
        _check(_lib.load().pesto_train_get_state(self._handle, None if w is None else w.ctypes.data, None if pr is None else pr.ctypes.data,
                                                 ctypes.byref(step), ctypes.byref(lr)))
        return w, pr, step.value, lr.value

    def blob(self):
        """The current weights as the flat float32 blob (pesto_amd.weights order)."""
        return self._get(weights=True)[0]

    def state_dict(self):
        return unflatten_blob(self.config, self.blob())

    @property
    def pos_ratios(self):
        """The running positive ratios per class (model/main.py:50), read back from the device."""
        return self._get(pos=True)[1]

    @pos_ratios.setter
    def pos_ratios(self, value):
        v = np.ascontiguousarray(_lib.host(value), dtype=np.float32).ravel()
        if v.size != self.config["dm"]["N2"]:
            raise ValueError(f"pos_ratios must have {self.config['dm']['N2']} entries, got {v.size}")
        _check(_lib.load().pesto_train_set_state(self._handle, v.ctypes.data, None, None))

    @property
    def global_step(self):
        return self._get()[2]

    @global_step.setter
    def global_step(self, value):
        _check(_lib.load().pesto_train_set_state(self._handle, None, ctypes.byref(ctypes.c_int64(int(value))), None))

    @property
    def lr(self):
        return self._get()[3]

    @lr.setter
    def lr(self, value):
        _check(_lib.load().pesto_train_set_state(self._handle, None, None, ctypes.byref(ctypes.c_float(float(value)))))

    def model(self, **kwargs):
        """A pesto_amd.Model loaded from the current weights, for fast inference (the MFMA path; the trainer itself keeps only the plain
        weight image)."""
        from .model import Model
        m = Model(self.config, device=self._gpu, **kwargs)
        m.load_blob(self.blob())
        return m

    def grads_dict(self, flat):
        """{state_dict key: array} views of a gradient in blob order."""
        out, off = {}, 0
        for key, shape in self._keys:
            n = int(np.prod(shape))
            out[key] = flat[off:off + n].reshape(shape)
            off += n
        return out

    def adam_step(self, grads):
        """torch.optim.Adam.step() with a gradient given in blob order (or as a {key: array} dict)."""
        if isinstance(grads, dict):
            grads = np.concatenate([np.asarray(_lib.host(grads[k]), np.float32).ravel() for k, _ in self._keys])
        g = np.ascontiguousarray(_lib.host(grads), dtype=np.float32).ravel()
        if g.size != self._n:
            raise ValueError(f"gradient has {g.size} values, the model has {self._n}")
        _check(_lib.load().pesto_train_adam(self._handle, g.ctypes.data))

    def set_timing(self, enabled=True):
        _check(_lib.load().pesto_train_set_timing(self._handle, 1 if enabled else 0))
        return self

    def timing(self):
        """{"forward_ms", "backward_ms", "adam_ms"} of the last train_step (HIP events; set_timing() first)."""
        ms = (ctypes.c_double * 3)()
        _check(_lib.load().pesto_train_get_timing(self._handle, ms))
        return {"forward_ms": ms[0], "backward_ms": ms[1], "adam_ms": ms[2]}

    # ------------------------------------------------------------------ the three steps
    def _segments(self, M):
        if isinstance(M, (tuple, list)) and len(M) == 2 and np.ndim(M[1]) == 0:
            return M[0], int(M[1])
        return mask_to_segments(M)

    def _step(self, mode, X, ids_topk, q, M, y):
        roa, R = self._segments(M)
        side = _lib.Side(X, self._gpu)
        ids = side.put(ids_topk, (np.int64, np.int32))
        if ids.ndim != 2:
            raise ValueError(f"ids_topk must be [N,k], got {list(ids.shape)}")
        N, k = int(ids.shape[0]), int(ids.shape[1])
        C = self.config["dm"]["N2"]
        X = side.put(X, np.float32, (N, 3), "X")
        q = side.put(q, np.float32, (N, self.config["em"]["N0"]), "q")
        roa = side.put(roa, np.int32, (N,), "res_of_atom")
        y = side.put(y, np.float32, name="y")
        if y.ndim != 2 or int(y.shape[0]) != R:
            raise _error(f"y must be [R,C] with R = {R}, got {list(y.shape)}")
        losses = side.empty((R, C), np.float32)
        p = side.empty((R, C), np.float32)
        z = side.empty((R, C), np.float32)
        grads = side.empty((self._n,), np.float32) if mode == MODE_GRAD else None
        _check(_lib.load().pesto_train_step(self._handle, mode, N, R, k, int(y.shape[1]), side.ptr(X), side.ptr(ids), _lib.ids_kind(ids), side.ptr(q),
                                            side.ptr(roa), side.ptr(y), side.ptr(losses), side.ptr(p), side.ptr(z), side.ptr(grads), side.kind, side.stream))
        self.last_z = side.result(z)      # the logits of the last step (the steps themselves return sigmoid(z), as eval_step does)
        if side.device is not None:
            self._last_call = (X, ids, q, roa, y)      # the launch reads them in stream order
        return side, losses, y, p, grads

    def eval_step(self, X, ids_topk, q, M, y):
        """(losses [R,C], y, sigmoid(z)) of model/main.py:42-58; pos_ratios is updated, nothing else."""
        side, losses, y, p, _ = self._step(MODE_EVAL, X, ids_topk, q, M, y)
        return side.result(losses), side.result(y), side.result(p)

    def loss_and_grad(self, X, ids_topk, q, M, y):
        """(losses, sigmoid(z), grads): eval_step plus the gradient of sum(losses) with respect to every parameter, as a dict
        {state_dict key: float32 array} (views of one flat array in blob order). The weights are not updated; pos_ratios is."""
        side, losses, y, p, grads = self._step(MODE_GRAD, X, ids_topk, q, M, y)
        return side.result(losses), side.result(p), self.grads_dict(side.result(grads))

    def train_step(self, X, ids_topk, q, M, y):
        """model/main.py:186-200: global_step += 1, forward, loss, backward, Adam. Returns (losses, y, sigmoid(z))."""
        side, losses, y, p, _ = self._step(MODE_TRAIN, X, ids_topk, q, M, y)
        return side.result(losses), side.result(y), side.result(p)

    # ------------------------------------------------------------------ stage entry points (tests)
    def stage_embed_bwd(self, q0, dq):
        q0 = np.ascontiguousarray(q0, np.float32)
        dq = np.ascontiguousarray(dq, np.float32)
        g = np.empty(self._n, np.float32)
        _check(_lib.load().pesto_train_stage_embed(self._handle, q0.shape[0], q0.ctypes.data, dq.ctypes.data, g.ctypes.data))
        return self.grads_dict(g)

    def stage_layer_bwd(self, layer, X, ids_topk, q_in, p_in, dq_out, dp_out):
        X = np.ascontiguousarray(X, np.float32)
        ids = np.ascontiguousarray(ids_topk, np.int32)
        N, k = ids.shape
        arrs = [np.ascontiguousarray(a, np.float32) for a in (q_in, p_in, dq_out, dp_out)]
        for a, w in zip(arrs, (32, 96, 32, 96)):
            if a.size != (N + 1) * w:
                raise ValueError("states and their gradients are [N+1,32] / [N+1,3,32] (with the sink row)")
        dq_in, dp_in, g = np.empty((N + 1, 32), np.float32), np.empty((N + 1, 3, 32), np.float32), np.empty(self._n, np.float32)
        _check(_lib.load().pesto_train_stage_layer(self._handle, int(layer), N, k, X.ctypes.data, ids.ctypes.data, _lib.IDS_INT32, *[a.ctypes.data for a in arrs],
                                                   dq_in.ctypes.data, dp_in.ctypes.data, g.ctypes.data))
        return dq_in, dp_in, self.grads_dict(g)

    def stage_head_bwd(self, q, p, res_of_atom, R, dz):
        q, p, dz = (np.ascontiguousarray(a, np.float32) for a in (q, p, dz))
        roa = np.ascontiguousarray(res_of_atom, np.int32)
        N = roa.size
        if q.size != N * 32 or p.size != N * 96 or dz.shape != (R, self.config["dm"]["N2"]):
            raise ValueError("q [N,32], p [N,3,32] (without the sink row), dz [R,n_out]")
        dq, dp, g = np.empty((N, 32), np.float32), np.empty((N, 3, 32), np.float32), np.empty(self._n, np.float32)
        _check(_lib.load().pesto_train_stage_head(self._handle, N, int(R), q.ctypes.data, p.ctypes.data, roa.ctypes.data, dz.ctypes.data, dq.ctypes.data,
                                                  dp.ctypes.data, g.ctypes.data))
        return dq, dp, self.grads_dict(g)


def _error(msg):
    err = _lib.PestoError(msg)
    err.code = -1
    return err


def scoring(eval_results):
    """model/main.py:61-79: eval_results = [(losses, y, p), ...] as the steps return them -> {"loss", "<c>/loss", "<c>/<score>"} with
    the scores of evaluate.bc_scoring (src/scoring.py:77-96), nan-averaged over the entries."""
    from .evaluate import BC_SCORE_NAMES, bc_scoring
    sum_losses, scores = [], []
    for losses, y, p in eval_results:
        sum_losses.append(_lib.host(losses).astype(np.float32).sum(0))
        scores.append(np.asarray(_lib.host(bc_scoring(y, p)), np.float32))
    m_losses = np.mean(np.stack(sum_losses, 0), 0)
    st = np.stack(scores, 0)
    cnt = np.sum(~np.isnan(st), 0)
    m_scores = np.where(cnt > 0, np.nansum(st, 0) / np.maximum(cnt, 1), np.nan)
    out = {"loss": float(np.sum(m_losses))}
    for i in range(m_losses.shape[0]):
        out[f"{i}/loss"] = m_losses[i]
        for j, name in enumerate(BC_SCORE_NAMES):
            out[f"{i}/{name}"] = m_scores[j, i]
    return out
