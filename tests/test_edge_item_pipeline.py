"""Item pipeline of the node-wave layer kernels: the rows of a wave's NEXT work item are requested while the current item runs.
Scheduling only - the logits must be the bits the kernels produced before the change.

Model: four layers, one each of nn = 8, 16, 32, 64, seeded synthetic weights, precision "f16_split". Every case runs in the three
work decompositions (pesto_debug_edge_mode 0 = chosen per launch, 1 = rendezvous, 2 = node waves on every layer) and is compared with
np.array_equal against tests/golden/edge_item_pipeline_parent.npz, recorded on the GPU by tests/golden/make_edge_item_pipeline_golden.py
from a build of the commit before the pipeline (rendezvous mode; the recorder asserts that the three modes of that build agree).

A node-wave launch has 256 workgroups of 8 item waves = 2,048 wave slots; a work item holds 2 / 1 / 2 / 1 centres at nn = 8 / 16 / 32 /
64 and a wave takes 1 / 2 / 1 / 2 items per iteration; smaller launches shrink the grid instead, so a wave has a successor item only
in launches of more than 2,048 items (nn = 8: above 4,096 atoms).
The atom counts walk the successor arithmetic of the item loop through its branches: one partly filled iteration (300), one full
round and a `tail` iteration with its wider stride (4,500), an odd number of centres so that the last nn = 8 tile holds one centre
(6,201), two and three full rounds plus a tail (9,000 / 13,001), and one collated batch whose structures cross the XCD shares.
"""
import numpy as np
import pytest

from conftest import golden

SIZES = (300, 4500, 6201, 9000, 13001)
BATCH = (1500, 2900, 1801)
MODES = (0, 1, 2)
GOLDEN_NAME = "edge_item_pipeline_parent"

_inputs = {}
_models = {}


def pipeline_config():
    from pesto_amd.config import make_config
    return make_config(30, [(8, 1), (16, 1), (32, 1), (64, 1)])


def case_names():
    return [f"n{n}" for n in SIZES] + ["batch_" + "_".join(str(s) for s in BATCH)]


def case_inputs(name):
    """(X, ids_topk 1-based, q0, res_of_atom, R, sizes or None) of a case; built once."""
    if name not in _inputs:
        from pesto_amd.topology import collate_batch_features, mask_to_segments, synthetic_structure
        if name.startswith("batch_"):
            structs = [list(synthetic_structure(n, 100 + 7 * b)) for b, n in enumerate(BATCH)]
            X, ids, q, M = collate_batch_features(structs)
            sizes = list(BATCH)
        else:
            n = int(name[1:])
            X, ids0, q, M = synthetic_structure(n, n)
            ids, sizes = np.asarray(ids0).astype(np.int64) + 1, None
        roa, R = mask_to_segments(np.asarray(M))
        _inputs[name] = (np.asarray(X), np.asarray(ids).astype(np.int64), np.asarray(q), np.asarray(roa).astype(np.int32), int(R), sizes)
    return _inputs[name]


def pipeline_model(mode):
    if mode not in _models:
        from pesto_amd import Model
        from pesto_amd.weights import synthetic_state_dict
        cfg = pipeline_config()
        m = Model(cfg, precision="f16_split")
        m.load_state_dict(synthetic_state_dict(cfg, seed=0))
        _models[mode] = m.debug_edge_mode(mode)
    return _models[mode]


def run_case(name, mode):
    X, ids, q, roa, R, sizes = case_inputs(name)
    return pipeline_model(mode).forward_segments(X, ids, q, roa, R, sizes=sizes)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", case_names())
def test_logits_are_the_parent_commits_bits(name, mode):
    ref = golden(GOLDEN_NAME)[name]
    z = run_case(name, mode)
    assert z.shape == ref.shape and np.isfinite(ref).all()
    assert np.array_equal(z, ref), (name, mode, int((z != ref).sum()), float(np.nanmax(np.abs(z - ref))))
