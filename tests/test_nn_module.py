"""pesto_amd.nn.Model as a torch Module, without a GPU: the reference's state_dict surface, and the refusal of CPU tensors (the library
is loaded at the first forward only)."""
import copy

import numpy as np
import pytest
import torch

from conftest import weights
from pesto_amd import _lib
from pesto_amd.config import CONFIGS, make_config
from pesto_amd.weights import blob_schema, blob_size, flatten_state_dict, unflatten_blob


@pytest.fixture(scope="module")
def model():
    from pesto_amd.nn import Model
    return Model(CONFIGS["i_v4_0"])


def test_state_dict_surface(model):
    cfg = CONFIGS["i_v4_0"]
    ref = unflatten_blob(cfg, np.zeros(blob_size(cfg), np.float32))
    sd = model.state_dict()
    assert set(sd) == set(ref)
    for k, v in ref.items():
        assert tuple(sd[k].shape) == tuple(np.shape(v)), k
        assert str(sd[k].dtype).replace("torch.", "") == str(np.asarray(v).dtype), k
    assert sd["sum.0.m_nn"].dtype == torch.int64 and sd["sum.0.su.sdk"].dtype == torch.float32
    names = [k for k, _ in model.named_parameters()]
    assert names == [k for k, _ in blob_schema(cfg)]      # blob order, every learned tensor once
    assert len(list(model.parameters())) == len(blob_schema(cfg))
    assert all(p.requires_grad and p.dtype == torch.float32 for p in model.parameters())
    assert isinstance(model, torch.nn.Module)


def test_load_state_dict_round_trip(model):
    sd = {k: torch.from_numpy(np.array(v)) for k, v in weights("i_v4_0").items()}
    res = model.load_state_dict(sd)      # strict
    assert not res.missing_keys and not res.unexpected_keys
    out = model.state_dict()
    for k, v in sd.items():
        assert torch.equal(out[k], v), k
    blob = flatten_state_dict(CONFIGS["i_v4_0"], {k: v.numpy() for k, v in out.items()})      # the library's own strict reader accepts it
    assert np.array_equal(blob, flatten_state_dict(CONFIGS["i_v4_0"], weights("i_v4_0")))
    bad = dict(sd); bad.pop("sum.3.su.evm.2.bias")
    with pytest.raises(RuntimeError):
        model.load_state_dict(bad)
    bad = dict(sd); bad["dm.4.weight"] = torch.zeros(4, 32)
    with pytest.raises(RuntimeError):
        model.load_state_dict(bad)


def test_module_behaviour(model):
    opt = torch.optim.Adam(model.parameters(), lr=1e-5)
    assert sum(len(g["params"]) for g in opt.param_groups) == len(blob_schema(CONFIGS["i_v4_0"]))
    assert model.train().training and not model.eval().training
    m2 = copy.deepcopy(model)
    m2.em.requires_grad_(False)
    frozen = [k for k, p in m2.named_parameters() if not p.requires_grad]
    assert frozen and all(k.startswith("em.") for k in frozen)
    assert all(p.requires_grad for p in model.parameters())      # the copy has parameters of its own
    assert m2.double().em._modules["0"].weight.dtype == torch.float64


def test_cpu_tensors_refused(model):
    N = 12
    X, ids, q, M = torch.zeros(N, 3), torch.zeros(N, 8, dtype=torch.int64), torch.zeros(N, 30), torch.ones(N, 1)
    with pytest.raises(_lib.PestoError, match="GPU"):
        model(X, ids, q, M)
    with pytest.raises(_lib.PestoError):
        with torch.no_grad():
            model(X, ids, q, (torch.zeros(N, dtype=torch.int32), 1))


def test_single_linear_variants_rejected():
    from pesto_amd.nn import Model
    cfg = copy.deepcopy(make_config(30, [(8, 1)]))
    cfg["em_depth"] = 1
    with pytest.raises(ValueError, match="em_depth"):
        Model(cfg)


def test_abi_has_the_autograd_entries():
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "pesto_hip.h")).read()
    declared = set(re.findall(r"\b(pesto_[a-z_]+)\s*\(", hdr))
    lib = _lib.load()
    for name in ("pesto_train_set_weights", "pesto_train_forward", "pesto_train_backward"):
        assert name in declared and name in _lib.ABI_SYMBOLS and hasattr(lib, name), name
