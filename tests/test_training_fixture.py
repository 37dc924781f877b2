"""Training checks that need no GPU: the fixtures agree with a NumPy restatement of the loss (model/main.py:49-58), their gradients are
laid out in blob order, and the trainer fails loudly without a device."""
import numpy as np
import pytest

from conftest import golden
from pesto_amd import _lib
from training_fixture import CONFIG, KEYS, case, loss_numpy, split, state_dict


@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_fixture_losses_match_numpy(name):
    (X, ids, q0, (roa, R), y), g = case(name)
    assert g["z"].shape == (R, 5) == y.shape and g["losses"].shape == (R, 5)
    losses, pos = loss_numpy(g["z"], y, np.full(5, 0.5), 0, dtype=np.float64)
    assert np.abs(pos - g["pos_ratios"]).max() <= 1e-6
    assert np.abs(losses - g["losses"]).max() <= 1e-6
    losses1, pos1 = loss_numpy(g["z"], y, np.full(5, 0.5), 1, dtype=np.float64)
    assert np.abs(pos1 - g["pos_ratios_step1"]).max() <= 1e-6 and np.abs(losses1 - g["losses_step1"]).max() <= 1e-6
    assert np.abs(pos - y.mean(0)).max() <= 1e-7      # global_step 0: the ratios are replaced by the batch's


def test_fixture_shapes():
    (X, ids, q0, (roa, R), y), g = case("A")
    assert X.shape[0] == 40 and ids.shape == (40, 64) and (ids[:, 40:] == 0).all()      # fewer than 64 atoms: zero-padded slots
    (X, ids, q0, (roa, R), y), g = case("B")
    assert list(g["sizes"]) == [200, 70] and X.shape[0] == 270 and ids[200:].min() > 200 and (y[:, 2] == 0).all()
    (X, ids, q0, (roa, R), y), g = case("C")
    assert list(g["sizes"]) == [64, 65, 8] and np.bincount(roa).min() == 1
    n = sum(int(np.prod(s)) for _, s in KEYS)
    for name in "ABC":
        gr = case(name)[1]["grads"]
        assert gr.size == n and np.isfinite(gr).all()
        d = split(gr)
        # a constant added to all logits of a softmax cancels: these five gradients are analytically zero
        scale = np.abs(gr).max()
        for k in [f"sum.{l}.su.eqkm.4.bias" for l in range(4)] + ["spl.sam.4.bias"]:
            assert np.abs(d[k]).max() <= 1e-6 * scale, k
    assert 0 < float(golden("training_curve")["deviation"]) < 1e-5


def test_trainer_without_gpu_fails_loudly(gpu_available):
    """Without a device the trainer must raise, never fall back to a CPU implementation."""
    if gpu_available:
        pytest.skip("a GPU is present")
    from pesto_amd.training import Trainer
    with pytest.raises(_lib.PestoError):
        Trainer(CONFIG, state_dict())


def test_trainer_rejects_single_linear_variants():
    from pesto_amd.config import CONFIGS
    from pesto_amd.training import Trainer
    with pytest.raises(ValueError, match="em_depth"):
        Trainer(CONFIGS["i_v3_1"], {})
