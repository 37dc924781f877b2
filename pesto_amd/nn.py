"""The reference's model as a differentiable ``torch.nn.Module`` on the MI355X: the training loop of model/main.py runs on it unchanged.

    from pesto_amd.nn import Model                       # instead of: from model import Model
    model = Model(config_model).to("cuda")
    model.load_state_dict(torch.load(".../model.pt"))     # the reference's keys, shapes and dtypes (strict)
    optimizer = torch.optim.Adam(model.parameters(), lr=1e-5)          # model/main.py:159
    z = model(X, ids_topk, q, M)                          # model/model.py:32-52, one collated batch
    loss.backward(); optimizer.step()                     # model/main.py:196-200, any loss, optimiser, schedule, frozen subset or clipping
    X.requires_grad_(); q.requires_grad_()                # d z / d X and d z / d q as on the reference (saliency, refinement)
    torch.save(model.state_dict(), path)                  # model/main.py:218; the reference loads it
    fast = model.inference_model()                        # the MFMA inference path (pesto_amd.Model) of the current weights

The parameters and buffers are built from ``weights.blob_schema`` by splitting the keys at the dots: the tree of containers carries the
reference's names without restating its module classes. ``forward`` runs through one autograd Function over the trainer handle of
libpesto_hip.so (pesto_train_set_weights / pesto_train_forward / pesto_train_backward, include/pesto_hip.h): the exact fp32 training
forward, which keeps the input state of every layer only when something requires a gradient, and the backward of pesto_amd.training
from the caller's dz. The parameters are concatenated into one flat tensor in blob order (``torch.cat`` is differentiable, so the flat
gradient finds its way back to every ``.grad``); the library's weight image is refreshed only when a parameter has changed.

One Module owns ONE workspace: a backward must follow its own forward. ``z1 = model(a); z2 = model(b); z1.sum().backward()`` raises
RuntimeError with the library's message instead of producing a gradient of the wrong forward (any later forward, also one under
``torch.no_grad()``, ends the earlier one; ``retain_graph=True`` on the last forward is fine and gives the same bits). Second derivatives
are not available (once_differentiable). Everything is float32 on one GPU; parameters or inputs on the CPU or in float64 raise
PestoError - there is no CPU fallback, as everywhere in this package.
"""
import ctypes

import numpy as np
import torch

from . import _lib
from .config import normalise
from .topology import mask_to_segments
from .weights import blob_schema, unflatten_blob


def _check(rc):
    _lib.check(rc, _lib.load().pesto_train_last_error)


def _error(msg):
    err = _lib.PestoError(msg)
    err.code = -1
    return err


class _Runtime:
    """The trainer handle of one Module (created at the first forward, on the parameters' GPU). Not copied with the Module: a deep copy
    or an unpickled Module creates its own at its first forward."""

    def __init__(self):
        self.handle, self.gpu, self.sig = None, None, None

    def __deepcopy__(self, memo):
        return _Runtime()

    def __reduce__(self):
        return (_Runtime, ())

    def close(self):
        if self.handle is not None:
            _lib.load().pesto_train_destroy(self.handle)
        self.handle, self.gpu, self.sig = None, None, None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _Forward(torch.autograd.Function):
    """z = model(X, ids_topk, q, M) with the states kept; backward: (dX, dq0, d flat) from dz."""

    @staticmethod
    def forward(ctx, module, X, ids, q, roa, R, flat):
        ctx.module = module
        ctx.save_for_backward(X, ids, q, roa)      # the library reads X, q and res_of_atom again in the backward: kept alive and unmodified
        ctx.shape = (int(X.shape[0]), int(q.shape[1]), int(flat.numel()))
        z, ctx.ticket = module._run(True, X, ids, q, roa, R)
        return z

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dz):
        N, n0, n = ctx.shape
        ctx.saved_tensors      # (raises if an input was modified in place since the forward)
        need_x, need_q, need_w = ctx.needs_input_grad[1], ctx.needs_input_grad[3], ctx.needs_input_grad[6]
        dz = dz.to(torch.float32).contiguous()
        dev = dz.device
        g = torch.empty(n, dtype=torch.float32, device=dev) if need_w else None
        dq0 = torch.empty((N, n0), dtype=torch.float32, device=dev) if need_q else None
        dX = torch.empty((N, 3), dtype=torch.float32, device=dev) if need_x else None
        ptr = lambda a: None if a is None else a.data_ptr()      # noqa: E731
        _check(_lib.load().pesto_train_backward(ctx.module._rt.handle, ctx.ticket, dz.data_ptr(), ptr(g), ptr(dq0), ptr(dX), _lib.PTR_DEVICE,
                                                torch.cuda.current_stream(dev).cuda_stream))
        return None, dX, None, dq0, None, None, g


class Model(torch.nn.Module):
    def __init__(self, config):
        super().__init__()
        self.config = normalise(config)
        if self.config["em_depth"] != 3 or self.config["dm_depth"] != 3:
            raise ValueError("training needs the three-Linear em and dm (em_depth = dm_depth = 3)")
        self._keys = blob_schema(self.config)
        self._slots = []      # (container, leaf name) of every parameter, in blob order
        gen = torch.Generator().manual_seed(0)
        for key, shape in self._keys:      # torch.nn.Linear's default range, U(-1/sqrt(fan_in), 1/sqrt(fan_in)); a bias follows its weight
            if len(shape) == 2:
                bound = 1.0 / float(np.sqrt(shape[1]))
            value = (torch.rand(shape, generator=gen) * 2.0 - 1.0) * bound
            parent, name = self._container(key)
            parent.register_parameter(name, torch.nn.Parameter(value))
            self._slots.append((parent, name))
        n = int(sum(int(np.prod(shape)) for _, shape in self._keys))
        for key, value in unflatten_blob(self.config, np.zeros(n, np.float32)).items():
            if key.endswith(".m_nn") or key.endswith(".su.sdk"):      # the two non-learned entries per layer (model_operations.py:85, 223)
                parent, name = self._container(key)
                parent.register_buffer(name, torch.from_numpy(np.array(value)))
        self._rt = _Runtime()

    def _container(self, key):
        """(module, leaf name) of a state_dict key; the containers on the way are created"""
        *path, name = key.split(".")
        mod = self
        for part in path:
            if part not in mod._modules:
                mod.add_module(part, torch.nn.Module())
            mod = mod._modules[part]
        return mod, name

    def _params(self):
        return [mod._parameters[name] for mod, name in self._slots]

    # ------------------------------------------------------------------ library calls
    def _prepare(self, params, flat, gpu):
        """the handle on the parameters' GPU, its weight image equal to the parameters"""
        rt = self._rt
        sig = tuple((p._version, p.data_ptr()) for p in params)
        if rt.handle is not None and rt.gpu == gpu and rt.sig == sig:
            return
        if flat is None:
            flat = torch.cat([p.detach().reshape(-1) for p in params])
        flat = flat.detach().contiguous()
        if rt.handle is None or rt.gpu != gpu:
            rt.close()
            blob = flat.cpu().numpy()
            cc = _lib.make_c_config(self.config, "fp32")
            h = ctypes.c_void_p()
            _check(_lib.load().pesto_train_create(ctypes.byref(cc), blob.ctypes.data, blob.size, gpu, 0.0, 0.5, ctypes.byref(h)))
            rt.handle, rt.gpu = h, gpu
        else:
            _check(_lib.load().pesto_train_set_weights(rt.handle, flat.data_ptr(), _lib.PTR_DEVICE, torch.cuda.current_stream(flat.device).cuda_stream))
        rt.sig = sig

    def _run(self, keep, X, ids, q, roa, R):
        z = torch.empty((R, self.config["dm"]["N2"]), dtype=torch.float32, device=X.device)
        ticket = ctypes.c_int64(0)
        _check(_lib.load().pesto_train_forward(self._rt.handle, 1 if keep else 0, int(X.shape[0]), R, int(ids.shape[1]), X.data_ptr(), ids.data_ptr(),
                                               _lib.ids_kind(ids), q.data_ptr(), roa.data_ptr(), z.data_ptr(), ctypes.byref(ticket), _lib.PTR_DEVICE,
                                               torch.cuda.current_stream(X.device).cuda_stream))
        return z, ticket.value

    def forward(self, X, ids_topk, q, M):
        """model/model.py:32-52 on one collated batch: X [N,3], ids_topk [N,k] (1-based, 0 = padding), q [N,n0], M the dense mask [N,R]
        or a pair (res_of_atom, R). Returns the logits z [R,n_out]."""
        params = self._params()
        for name, a in (("X", X), ("ids_topk", ids_topk), ("q", q)):
            if not (torch.is_tensor(a) and a.is_cuda):
                raise _error(f"{name} must be a tensor on the GPU (pesto_amd.nn has no CPU path)")
        dev = X.device
        for name, a in [("X", X), ("q", q)] + [(k, p) for (k, _), p in zip(self._keys, params)]:
            if a.device != dev:
                raise _error(f"{name} is on {a.device}, X is on {dev}: parameters and inputs must be on one GPU (use .to())")
            if a.dtype != torch.float32:
                raise _error(f"{name} is {a.dtype}: pesto_amd.nn is float32 only")
        if ids_topk.device != dev or ids_topk.dtype not in (torch.int64, torch.int32) or ids_topk.ndim != 2:
            raise _error(f"ids_topk must be an int64 or int32 tensor [N,k] on {dev}")
        N = int(ids_topk.shape[0])
        n0 = self.config["em"]["N0"]
        if tuple(X.shape) != (N, 3) or tuple(q.shape) != (N, n0):
            raise _error(f"X must be [{N},3] and q [{N},{n0}], got {list(X.shape)} and {list(q.shape)}")
        if isinstance(M, (tuple, list)) and len(M) == 2 and np.ndim(M[1]) == 0:
            roa, R = M[0], int(M[1])
        else:
            roa, R = mask_to_segments(M)
        roa = torch.as_tensor(roa).to(device=dev, dtype=torch.int32).contiguous()
        if tuple(roa.shape) != (N,):
            raise _error(f"res_of_atom must be [{N}], got {list(roa.shape)}")
        need = torch.is_grad_enabled() and (X.requires_grad or q.requires_grad or any(p.requires_grad for p in params))
        flat = torch.cat([p.reshape(-1) for p in params]) if need else None
        self._prepare(params, flat, dev.index if dev.index is not None else torch.cuda.current_device())
        Xc, idsc, qc = X.contiguous(), ids_topk.contiguous(), q.contiguous()
        if not need:
            return self._run(False, Xc.detach(), idsc, qc.detach(), roa, R)[0]
        return _Forward.apply(self, Xc, idsc, qc, roa, R, flat)

    def inference_model(self, **kwargs):
        """A pesto_amd.Model loaded from the current weights, for fast inference (the MFMA path), like Trainer.model()."""
        from .model import Model as InferenceModel
        params = self._params()
        dev = params[0].device
        m = InferenceModel(self.config, device=dev.index if dev.type == "cuda" else 0, **kwargs)
        m.load_blob(torch.cat([p.detach().reshape(-1) for p in params]).to(torch.float32).cpu().numpy())
        return m
