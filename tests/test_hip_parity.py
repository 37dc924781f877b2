"""GPU parity tests (-m gpu): the HIP path, called through the C ABI, against (a) golden vectors captured from the
reference PyTorch CPU path and (b) the CPU oracle on the same seeded inputs.
Tolerances: whole forward 1e-4 abs on z (the north-star's fp32 bound; measured 1-3e-5); per stage 1e-5 abs for the
small stages and 1e-6 of the state scale for a layer (see stage_tol)."""
import functools

import numpy as np
import pytest

from conftest import CFG4_CHAINS, cfg4_structure, golden, onehot, weights
from pesto_amd.config import CONFIGS

pytestmark = pytest.mark.gpu


_IMPL = {"name": "mfma"}
# layer implementation -> (Model precision, pesto_debug_select layer_kernels)
_IMPL_ARGS = {"mfma": ("auto", 0), "mfma_exact": ("fp32", 0), "v1": ("auto", 1)}


@pytest.fixture(params=["mfma", "mfma_exact", "v1"])
def impl(request):
    """All layer implementations: the shipped MFMA path (hybrid first layer, big GEMMs on f16-split MFMA, finish phase inside the
    edge kernel, precision "auto"), the exact fp32 MFMA kernels (precision "fp32" - also what "auto" falls back to) and the
    LDS-tiled fp32 VALU kernel (debug twin 1)."""
    _IMPL["name"] = request.param
    yield request.param
    _IMPL["name"] = "mfma"


def stage_tol(ref):
    """Per-stage bound: 1e-6 relative to the largest reference magnitude (+1e-6): a few fp32 ulps of the state scale.
    (States reach |p| ~ 27 at layer 15; a fixed 1e-5 would be 0.4 ppm of that, below fp32 re-association noise.)"""
    return 1e-6 * (1.0 + float(np.abs(ref).max()))


def _model(tag, impl=None):
    from pesto_amd import Model
    precision, twin = _IMPL_ARGS[impl or _IMPL["name"]]
    m = Model(CONFIGS[tag], precision=precision).debug_select(twin)
    m.load_state_dict(weights(tag))
    # these tests pin the KERNELS (bit identities between launch shapes, staged and fused chains, batch and single calls), several of them on
    # structures of fewer than 64 atoms: "auto"'s pad trigger (pesto_set_auto_pad_trigger: such structures are repeated on the exact
    # kernels) is a policy on top and is tested in tests/test_fuzz_pins.py - off here
    return m.set_auto_pad_trigger(False).eval()


def _oracle(tag):
    from oracle import oracle
    return oracle.OracleModel(CONFIGS[tag], weights(tag))


def test_stage_embed_unpack():
    g = golden("ops_i_v4_0_crop200")
    m = _model("i_v4_0")
    q = m.stage_embed(onehot(g["em_in_idx"], 30))
    assert np.abs(q - g["em_out"]).max() < 1e-6
    for ids in (g["ids_topk"].astype(np.int32), g["ids_topk"].astype(np.int64)):
        D, R = m.stage_unpack(g["X"], ids)
        assert np.abs(D - g["D_nn"]).max() < 1e-5
        assert np.abs(R - g["R_nn"]).max() < 1e-6
        assert np.all(D[0] == 0) and np.all(R[0] == 0)


@pytest.mark.parametrize("layer", [0, 3, 4, 8, 12, 15])
def test_stage_layer(layer, impl):
    g = golden("ops_i_v4_0_crop200")
    m = _model("i_v4_0")
    m.stage_unpack(g["X"], g["ids_topk"].astype(np.int32))
    q, p = m.stage_layer(layer, g[f"L{layer}_q_in"], g[f"L{layer}_p_in"])
    assert np.abs(q - g[f"L{layer}_q_out"]).max() < stage_tol(g[f"L{layer}_q_out"])
    assert np.abs(p - g[f"L{layer}_p_out"]).max() < stage_tol(g[f"L{layer}_p_out"])
    assert np.all(q[0] == 0) and np.all(p[0] == 0)


def test_stage_pool_decode():
    g = golden("ops_i_v4_0_crop200")
    m = _model("i_v4_0")
    roa = g["res_of_atom"]
    qr, pr, z = m.stage_pool(g["L15_q_out"][1:], g["L15_p_out"][1:], roa, int(roa.max()) + 1)
    assert np.abs(qr - g["pool_qr"]).max() < 1e-5
    assert np.abs(pr - g["pool_pr"]).max() < 1e-5
    assert np.abs(z - g["z"]).max() < 1e-5


@pytest.mark.parametrize("fixture", ["fwd_i_v4_0_2CUA", "edge_n40", "fwd_i_v4_0_2AYO"])
def test_prepare_phase_in_the_edge_kernel_equals_the_node_kernel_bitwise(fixture):
    """The forward runs ONE node launch; every later layer's records come from the prepare phase of the previous edge launch. The
    staged chain (pesto_stage_layer: node kernel + edge kernel per layer, no prepare phase) must give the same bits: the prepare phase
    restates k_node16's arithmetic on the state the finish phase has just computed (955 atoms: eight-wave workgroups, one tile per
    rendezvous; 40: wrap-around rows; 2,810: twelve-wave workgroups at nn = 64, twelve-wave fine items at nn = 16 / 32)."""
    g = golden(fixture)
    m = _model("i_v4_0", "mfma")
    roa = g["res_of_atom"]
    R = int(roa.max()) + 1
    ids = g["ids_topk"].astype(np.int32)
    q0 = onehot(g["q_idx"], 30)
    z = m.forward_segments(g["X"], ids, q0, roa, R)
    q = np.concatenate([np.zeros((1, 32), np.float32), m.stage_embed(q0)])
    p = np.zeros((q.shape[0], 3, 32), np.float32)
    m.stage_unpack(g["X"], ids)
    for layer in range(len(CONFIGS["i_v4_0"]["sum"])):
        q, p = m.stage_layer(layer, q, p)
    _, _, z_staged = m.stage_pool(q[1:], p[1:], roa, R)
    assert np.array_equal(z, z_staged)


@pytest.mark.parametrize("tag,fixture", [
    ("i_v4_0", "fwd_i_v4_0_2CUA"), ("i_v4_0", "fwd_i_v4_0_2AYO"), ("i_v3_0", "fwd_i_v3_0_2CUA"), ("i_v3_1", "fwd_i_v3_1h_2CUA"),
    ("i_v4_0", "edge_n40"), ("i_v4_0", "edge_batch2"), ("i_v4_0", "edge_coincident"), ("i_v4_0", "edge_single_atom_residue"),
])
def test_forward_golden(tag, fixture, impl):
    g = golden(fixture)
    m = _model(tag)
    roa = g["res_of_atom"]
    z = m.forward_segments(g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], CONFIGS[tag]["em"]["N0"]), roa, int(roa.max()) + 1)
    assert z.shape == g["z"].shape and np.isfinite(z).all()
    assert np.abs(z - g["z"]).max() < 1e-4


def test_forward_i_v4_1_32_layers():
    """BASELINE configs 1 and 2 geometry with the i_v4_1 architecture (stacked real weights)."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    m = _model("i_v4_1")
    for inputs, out in (("fwd_i_v4_0_2CUA", "fwd_i_v4_1_stacked_2CUA"), ("fwd_i_v4_0_2AYO", "fwd_i_v4_1_stacked_2AYO")):
        g = golden(inputs)
        roa = g["res_of_atom"]
        z = m.forward_segments(g["X"], g["ids_topk"], onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)
        assert np.abs(z - golden(out)["z"]).max() < 1e-4
    for n in (512, 3000):
        gs = golden(f"fwd_i_v4_1_stacked_synth{n}")
        X, _, q, M = synthetic_structure(n, int(gs["seed"]))
        roa, R = mask_to_segments(M)
        z = m.forward_segments(X, gs["ids_topk"].astype(np.int32), q, roa, R)
        assert np.abs(z - gs["z"]).max() < 1e-4


def test_reference_call_signature_torch_cpu_and_device():
    """Model(config).forward(X, ids_topk, q, M) with torch tensors, CPU and ROCm, as apply_model.ipynb:155 calls it."""
    import torch
    g = golden("fwd_i_v4_0_2CUA")
    roa = g["res_of_atom"]
    R = int(roa.max()) + 1
    M = np.zeros((roa.size, R), np.float32)
    M[np.arange(roa.size), roa] = 1
    args = [torch.from_numpy(g["X"]), torch.from_numpy(g["ids_topk"].astype(np.int64)), torch.from_numpy(onehot(g["q_idx"], 30)), torch.from_numpy(M)]
    m = _model("i_v4_0")
    z_cpu = m(*args)
    assert isinstance(z_cpu, torch.Tensor) and z_cpu.device.type == "cpu"
    assert (z_cpu - torch.from_numpy(g["z"])).abs().max() < 1e-4
    dev = torch.device("cuda:0")
    m = m.to(dev)
    z_dev = m(*[a.to(dev) for a in args])
    assert z_dev.is_cuda and z_dev.dtype == torch.float32
    assert torch.equal(z_dev.cpu(), z_cpu)     # same kernels, same order -> bitwise
    # a side stream
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        z2 = m(*[a.to(dev) for a in args])
    s.synchronize()
    assert torch.equal(z2.cpu(), z_cpu)


def test_oracle_vs_hip_seeded_random_structures():
    """HIP path vs the CPU oracle on seeded synthetic clouds of ragged sizes, batched (block-diagonal collation)."""
    from pesto_amd.topology import collate_batch_features, mask_to_segments, synthetic_structure
    m, o = _model("i_v4_0"), _oracle("i_v4_0")
    batch = [list(synthetic_structure(n, seed)) for n, seed in ((65, 1), (130, 2), (257, 3))]
    X, ids, q, M = collate_batch_features(batch)
    roa, R = mask_to_segments(M)
    z_h = m.forward_segments(X, ids, q, roa, R)
    z_o = o.forward_segments(X, ids, q, roa, R)
    assert np.abs(z_h - z_o).max() < 1e-4


def test_rotation_translation_invariance():
    """Oracle-free property the reference holds to 2.1e-5: rigid motion of X, same ids -> same z."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    m = _model("i_v4_0")
    X, ids, q, M = synthetic_structure(600, 9)
    ids1 = ids + 1
    roa, R = mask_to_segments(M)
    z0 = m.forward_segments(X, ids1, q, roa, R)
    rng = np.random.default_rng(0)
    Q, _ = np.linalg.qr(rng.normal(size=(3, 3)))
    X2 = (X.astype(np.float64) @ Q.T + np.array([11.0, -7.0, 3.0])).astype(np.float32)
    z1 = m.forward_segments(X2, ids1, q, roa, R)
    assert np.abs(z0 - z1).max() < 1e-4


def test_bad_inputs_raise():
    from pesto_amd._lib import PestoError
    g = golden("edge_n40")
    m = _model("i_v4_0")
    roa = g["res_of_atom"]
    ids = g["ids_topk"].astype(np.int64).copy()
    ids[3, 2] = 1000
    with pytest.raises(PestoError):
        m.forward_segments(g["X"], ids, onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)
    # the handle survives a failed structure (interfaceome/apply_model.py:57-82 skips and continues)
    z = m.forward_segments(g["X"], g["ids_topk"], onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)
    assert np.abs(z - g["z"]).max() < 1e-4


def test_forward_i_v3_0_synthetic_123_features():
    """BASELINE config 3 shape: i_v3_0 (16 layers, 30+29+64 one-hots) on a synthetic cloud, real weights."""
    from pesto_amd.topology import extract_topology, mask_to_segments, synthetic_structure
    gs = golden("fwd_i_v3_0_synth512")
    X, ids0, q, M = synthetic_structure(512, int(gs["seed"]), n0=123)
    roa, R = mask_to_segments(M)
    z = _model("i_v3_0").forward_segments(X, ids0 + 1, q, roa, R)
    assert np.abs(z - gs["z"]).max() < 1e-4


def test_large_structure_config5_vs_oracle():
    """BASELINE config 5: one N=20,000-atom structure (R=2,500), i_v4_1 architecture; segmented pool, no dense [N,R] mask.
    Checked against the CPU oracle on the same inputs (a few seconds on the GPU box's host cores)."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    X, ids0, q, M = synthetic_structure(20000, 5)
    roa, R = mask_to_segments(M)
    assert R == 2500
    ids = (ids0 + 1).astype(np.int32)
    z = _model("i_v4_1").forward_segments(X, ids, q, roa, R)
    assert z.shape == (2500, 5) and np.isfinite(z).all()
    z_ref = _oracle("i_v4_1").forward_segments(X, ids, q, roa, R)
    assert np.abs(z - z_ref).max() < 1e-4


def test_determinism_bitwise():
    """No float atomics anywhere: two runs of the same batch give identical bits (needed for 1-GPU == N-GPU results)."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    X, ids0, q, M = synthetic_structure(700, 21)
    roa, R = mask_to_segments(M)
    m = _model("i_v4_1")
    z0 = m.forward_segments(X, ids0 + 1, q, roa, R)
    z1 = m.forward_segments(X, ids0 + 1, q, roa, R)
    assert np.array_equal(z0, z1)


# ------------------------------------------------------------------ GPU k-NN topology + collate
def _check_same_neighbours(ids, ref, X, offset=0):
    """Exact match, or - where the reference's sort keys tie - the same keys in the same order. Keys follow the reference
    rule D + max(D) * (D < 1e-2) (src/data_encoding.py:93): e.g. self (key = max(D)) ties with the farthest atom of the
    structure, and torch.topk / argsort may legitimately keep either one."""
    if np.array_equal(ids, ref):
        return
    assert np.array_equal((ids > 0), (ref > 0))
    D = np.sqrt(((X[None, :, :] - X[:, None, :]) ** 2).sum(2, dtype=np.float32)).astype(np.float32)
    K = D + D.max() * (D < 1e-2)
    rows = np.arange(X.shape[0])[:, None]
    k_a = np.where(ids > 0, K[rows, np.maximum(ids - 1 - offset, 0)], 0)
    k_b = np.where(ref > 0, K[rows, np.maximum(ref - 1 - offset, 0)], 0)
    assert np.allclose(k_a, k_b, rtol=0, atol=2e-6)
    assert np.mean(ids != ref) < 0.01


def test_knn_matches_reference_extract_topology():
    m = _model("i_v4_0")
    g = golden("topology_synth300")
    ids = m.knn_collate(g["X"], [300])
    assert ids.shape == (300, 64) and ids.dtype == np.int64
    assert np.array_equal(ids, g["ids_topk0"].astype(np.int64) + 1)
    g = golden("topology_synth50")                           # N < 64: knn = N, self sorted to the far end, zero padding
    ids = m.knn_collate(g["X"], [50])
    assert np.all(ids[:, 50:] == 0) and np.all(ids[:, :50] > 0)
    assert np.array_equal(ids[:, :48], g["ids_topk0"][:, :48].astype(np.int64) + 1)
    assert np.array_equal(np.sort(ids[:, :50], 1), np.sort(g["ids_topk0"].astype(np.int64) + 1, 1))


def test_knn_collate_matches_reference_batch_fixture():
    g = golden("edge_batch2")                               # reference extract_topology + collate_batch_features on 300 + 40 atoms
    (n0, r0), (n1, r1) = g["sizes"]
    m = _model("i_v4_0")
    ids = m.knn_collate(g["X"], [n0, n1])
    ref = g["ids_topk"].astype(np.int64)
    assert np.array_equal(ids[:n0], ref[:n0])
    assert np.array_equal(ids[n0:, :n1 - 2], ref[n0:, :n1 - 2]) and np.all(ids[n0:, n1:] == 0)
    assert np.array_equal(np.sort(ids[n0:], 1), np.sort(ref[n0:], 1))


def test_knn_ragged_batch_with_coincident_atoms_vs_host_contract():
    from pesto_amd.topology import collate_batch_features, extract_topology, synthetic_cloud
    sizes = [65, 700, 64, 33, 1200]
    Xs = [synthetic_cloud(n, 40 + k) for k, n in enumerate(sizes)]
    Xs[1][17] = Xs[1][400]                                   # exactly coincident pair
    Xs[4][5] = Xs[4][900] + np.float32(2e-3)                 # within the 1e-2 mask
    batch = [[x, extract_topology(x, 64), np.zeros((x.shape[0], 30), np.float32), np.ones((x.shape[0], 1), bool)] for x in Xs]
    Xc, ref, _, _ = collate_batch_features(batch)
    m = _model("i_v4_0")
    ids = m.knn_collate(Xc, sizes)
    off = 0
    for n in sizes:
        _check_same_neighbours(ids[off:off + n], ref[off:off + n], Xc[off:off + n], offset=off)
        off += n
    import torch
    ids_dev = m.to("cuda:0").knn_collate(torch.from_numpy(Xc).cuda(), sizes)
    assert ids_dev.is_cuda and torch.equal(ids_dev.cpu(), torch.from_numpy(ids))


def test_host_arrays_beside_a_rocm_lead_go_to_its_gpu():
    """X decides where forward_segments / knn_tie_rows run (pesto_amd._lib.Side): with a ROCm X, ids_topk / q0 / res_of_atom given as numpy
    arrays or CPU tensors are copied to its GPU, never passed on as host pointers - the bits of the all-device call, which are the bits of
    the host call. The headline's ROCm inputs are used as they are."""
    import torch
    from pesto_amd import _lib
    g = golden("fwd_i_v4_0_2CUA")
    X, ids, q, roa = g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 30), g["res_of_atom"].astype(np.int32)
    n, R = X.shape[0], int(g["res_of_atom"].max()) + 1
    m = _model("i_v4_0").to("cuda:0")
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")
    Xd, idsd = d(X), d(ids)
    side = _lib.Side(Xd, 0)
    assert side.put(Xd, np.float32, (n, 3)) is Xd and side.put(idsd, (np.int64, np.int32)) is idsd      # no copy, no kernel
    for sizes in (None, [n]):                                   # pesto_forward / pesto_forward_structures
        z_host = m.forward_segments(X, ids, q, roa, R, sizes=sizes)
        z_dev = m.forward_segments(Xd, idsd, d(q), d(roa), R, sizes=sizes)
        assert np.array_equal(z_dev.cpu().numpy(), z_host)
        for ids_, q_, roa_ in ((ids, q, roa), (torch.from_numpy(ids), torch.from_numpy(q), torch.from_numpy(roa)),
                               (ids.astype(np.int32), q.astype(np.float64), roa.tolist())):
            z_mix = m.forward_segments(Xd, ids_, q_, roa_, R, sizes=sizes)
            assert z_mix.is_cuda and torch.equal(z_mix, z_dev)
    ids_k = m.knn_collate(X, [n])
    fl_host = m.knn_tie_rows(X, [n], ids_k)
    fl_dev = m.knn_tie_rows(Xd, [n], d(ids_k))
    assert fl_dev.is_cuda and np.array_equal(fl_dev.cpu().numpy(), fl_host)
    for ids_ in (ids_k, torch.from_numpy(ids_k), ids_k.astype(np.int32)):
        assert torch.equal(m.knn_tie_rows(Xd, [n], ids_), fl_dev)


def test_knn_feeds_forward_end_to_end():
    """kNN on the GPU -> forward on the GPU gives the reference golden z (inputs: coordinates only, no host topology)."""
    g = golden("fwd_i_v4_0_2CUA")
    m = _model("i_v4_0")
    ids = m.knn_collate(g["X"], [g["X"].shape[0]])
    roa = g["res_of_atom"]
    z = m.forward_segments(g["X"], ids, onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)
    assert np.abs(z - g["z"]).max() < 1e-4


# ---------------------------------------------------------------------------------------------- trajectory frames
def test_frames_match_reference_md_loop_golden():
    """forward_frames == the reference's per-frame loop with frame-0 topology (md_analysis/apply_model_md.ipynb cell 6),
    in the notebook's own [N, frames, 3] layout (strided, read in place)."""
    g = golden("frames_i_v4_0_2CUA")
    m = _model("i_v4_0")
    q = onehot(g["q_idx"], 30)
    R = g["z"].shape[1]
    z = m.forward_frames_segments(g["X_traj"], g["ids_topk"], q, g["res_of_atom"], R, frame_axis=1)
    assert z.shape == g["z"].shape
    assert np.abs(z - g["z"]).max() < 1e-4
    # bit-identical to separate single-frame calls, whatever the launch grouping
    singles = np.stack([m.forward_segments(np.ascontiguousarray(g["X_traj"][:, f]), g["ids_topk"], q, g["res_of_atom"], R)
                        for f in range(z.shape[0])])
    assert np.array_equal(z, singles)
    for fpl in (1, 3):
        assert np.array_equal(m.forward_frames_segments(g["X_traj"], g["ids_topk"], q, g["res_of_atom"], R, 1, fpl), singles)


def test_frames_on_real_md_conformations():
    """The trajectory path on REAL conformations: 29 MD cluster representatives of one molecule (the reference's
    md_analysis/pdbs_clusters/1JTG_uL_*), frame-0 topology for every frame as md_analysis/apply_model_md.ipynb cell 6 does, trained
    i_v4_0 - against the reference's per-frame loop, and bit-identical to separate single-frame calls."""
    from conftest import md_frames
    f = md_frames()
    m = _model("i_v4_0")
    z = m.forward_frames_segments(f["X_frames"], f["ids"], f["q0"], f["res_of_atom"], f["R"])
    assert z.shape == f["z"].shape and z.shape[0] == 29
    assert np.abs(z - f["z"]).max() < 1e-4, float(np.abs(z - f["z"]).max())
    singles = np.stack([m.forward_segments(np.ascontiguousarray(f["X_frames"][i]), f["ids"], f["q0"], f["res_of_atom"], f["R"]) for i in (0, 7, 28)])
    assert np.array_equal(z[[0, 7, 28]], singles)


def test_frames_small_structure_per_frame_wrap_and_max():
    """N < 64: padded ids wrap to the last atom OF THE FRAME and max(D) is per frame (per call in the reference)."""
    g = golden("frames_i_v4_0_n40")
    m = _model("i_v4_0")
    q = onehot(g["q_idx"], 30)
    z = m.forward_frames_segments(g["X_frames"], g["ids_topk"].astype(np.int64), q, g["res_of_atom"], g["z"].shape[1])
    assert np.abs(z - g["z"]).max() < 1e-4


def test_frames_device_tensors_strided_view():
    import torch
    g = golden("frames_i_v4_0_2CUA")
    m = _model("i_v4_0").to("cuda")
    R = g["z"].shape[1]
    M = np.zeros((g["X_traj"].shape[0], R), np.float32)
    M[np.arange(M.shape[0]), g["res_of_atom"]] = 1.0
    Xt = torch.from_numpy(g["X_traj"]).cuda()                      # [N, F, 3] as in the notebook
    z = m.forward_frames(Xt, torch.from_numpy(g["ids_topk"].astype(np.int64)).cuda(), torch.from_numpy(onehot(g["q_idx"], 30)).cuda(),
                         torch.from_numpy(M).cuda(), frame_axis=1)
    assert z.is_cuda and tuple(z.shape) == g["z"].shape
    assert np.abs(z.cpu().numpy() - g["z"]).max() < 1e-4
    z2 = m.forward_frames(Xt.transpose(0, 1)[1:3], torch.from_numpy(g["ids_topk"]).cuda(), torch.from_numpy(onehot(g["q_idx"], 30)).cuda(),
                          torch.from_numpy(M).cuda(), frame_axis=0)   # a non-contiguous [F', N, 3] view
    assert torch.equal(z2, z[1:3])
    z_host = m.forward_frames(g["X_traj"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 30), M, frame_axis=1)   # from host memory
    assert isinstance(z_host, np.ndarray) and np.array_equal(z.cpu().numpy(), z_host)


def test_frames_bad_arguments():
    from pesto_amd._lib import PestoError
    g = golden("frames_i_v4_0_n40")
    m = _model("i_v4_0")
    q = onehot(g["q_idx"], 30)
    with pytest.raises(ValueError):
        m.forward_frames_segments(g["X_frames"][:, :30], g["ids_topk"], q, g["res_of_atom"], g["z"].shape[1])
    bad = g["ids_topk"].copy()
    bad[3, 2] = 41                                                  # > N: would alias an atom of the NEXT frame in the batch
    with pytest.raises(PestoError):
        m.forward_frames_segments(g["X_frames"], bad, q, g["res_of_atom"], g["z"].shape[1])
    z = m.forward_frames_segments(g["X_frames"], g["ids_topk"], q, g["res_of_atom"], g["z"].shape[1])   # handle still usable
    assert np.abs(z - g["z"]).max() < 1e-4


# ---------------------------------------------------------------------------------------------- post-processing
def test_postprocess_matches_reference_sigmoid_and_encode_bfactor():
    import torch
    g = golden("frames_i_v4_0_2CUA")
    m = _model("i_v4_0")
    p, bf = m.postprocess(g["z"][0], g["res_of_atom"])
    assert np.abs(p - g["p0"]).max() < 1e-6          # same z in: only the exp implementation differs
    assert bf.shape == g["bfactor0"].shape and np.abs(bf - g["bfactor0"]).max() < 1e-6
    assert np.array_equal(bf, p[g["res_of_atom"]].T)
    # end to end on device tensors: forward -> sigmoid -> atoms, nothing leaves the GPU in between
    m = m.to("cuda")
    q = onehot(g["q_idx"], 30)
    R = g["z"].shape[1]
    M = np.zeros((q.shape[0], R), np.float32)
    M[np.arange(M.shape[0]), g["res_of_atom"]] = 1.0
    Md = torch.from_numpy(M).cuda()
    z = m(torch.from_numpy(np.ascontiguousarray(g["X_traj"][:, 0])).cuda(), torch.from_numpy(g["ids_topk"].astype(np.int64)).cuda(),
          torch.from_numpy(q).cuda(), Md)
    p, bf = m.postprocess(z, Md)
    assert p.is_cuda and bf.is_cuda
    assert np.abs(p.cpu().numpy() - g["p0"]).max() < 1e-5     # 1e-5 on sigmoid(z)
    assert np.abs(bf.cpu().numpy() - g["bfactor0"]).max() < 1e-5
    p_only, none = m.postprocess(z)
    assert none is None and torch.equal(p_only, p)
    p_host, bf_host = m.postprocess(z.cpu().numpy(), M)                 # the same call from host memory: the same bits
    assert np.array_equal(p.cpu().numpy(), p_host) and np.array_equal(bf.cpu().numpy(), bf_host)


# ---------------------------------------------------------------------------------------------- apply_model.ipynb cell 6, natively
def test_apply_model_chain_pdb_to_bfactor_pdb(tmp_path):
    """PDB text -> native read/clean/encode -> GPU k-NN -> forward -> GPU sigmoid/expansion -> native b-factor PDB, against the
    same chain assembled from the checked pieces (host topology contract, CPU oracle, numpy sigmoid)."""
    import gzip
    import os
    from conftest import GOLDEN
    from pesto_amd.structure_io import Structure
    from pesto_amd.topology import extract_topology
    text = gzip.open(os.path.join(GOLDEN, "pdb", "7KHT_lipid.pdb.gz"), "rt").read()
    s = Structure.parse_pdb(text).preprocess()
    X, q, roa, R = s.encode(30)
    m = _model("i_v4_0")
    ids = m.knn_collate(X, [len(s)])
    ids_host = extract_topology(X, 64) + 1
    _check_same_neighbours(ids, ids_host, X)
    z = m.forward_segments(X, ids, q, roa, R)
    zo = _oracle("i_v4_0").forward_segments(X, ids.astype(np.int32), q, roa, R)
    assert np.abs(z - zo).max() < 1e-4
    p, bf = m.postprocess(z, roa)
    assert np.abs(p - 1.0 / (1.0 + np.exp(-zo.astype(np.float64)))).max() < 1e-5
    out = tmp_path / "7KHT_lipid_i0.pdb"
    s.save_pdb(str(out), bf[0])
    lines = out.read_text().split("\n")
    want = gzip.open(os.path.join(GOLDEN, "pdb", "7KHT_lipid_i0.pdb.gz"), "rt").read().split("\n")
    assert len(lines) == len(want)
    atoms = [l for l in lines if l.startswith(("ATOM", "HETATM"))]
    assert [l[:54] for l in atoms] == [l[:54] for l in want if l.startswith(("ATOM", "HETATM"))]
    assert [float(l[54:60]) for l in atoms] == [float("%.2f" % v) for v in bf[0]]


# ---------------------------------------------------------------------------------------------- list of structures
def _split_batch_fixture(g):
    """Undo collate_batch_features on the edge_batch2 fixture: per-structure (X, 0-based ids [N_b, min(64, N_b)], q0, M)."""
    out, a0, r0 = [], 0, 0
    for n, r in g["sizes"]:
        n, r = int(n), int(r)
        kb = min(64, n)
        ids0 = g["ids_topk"][a0:a0 + n, :kb].astype(np.int64) - a0 - 1
        roa = g["res_of_atom"][a0:a0 + n] - r0
        M = np.zeros((n, r), np.float32)
        M[np.arange(n), roa] = 1.0
        out.append((g["X"][a0:a0 + n], ids0, onehot(g["q_idx"][a0:a0 + n], 30), M))
        a0 += n; r0 += r
    return out


def test_forward_batch_collates_on_device_like_the_reference():
    from pesto_amd._lib import PestoError
    g = golden("edge_batch2")                      # reference collate_batch_features + forward on 300 + 40 atoms
    m = _model("i_v4_0")
    structs = _split_batch_fixture(g)
    zs = m.forward_batch(structs)
    assert [z.shape[0] for z in zs] == [int(r) for _, r in g["sizes"]]
    z = np.concatenate(zs, 0)
    assert np.abs(z - g["z"]).max() < 1e-4
    zc = m.forward_segments(g["X"], g["ids_topk"], onehot(g["q_idx"], 30), g["res_of_atom"], g["z"].shape[0])
    assert np.array_equal(z, zc)                   # same kernels on the same collated arrays
    z32 = m.forward_batch([(X, ids.astype(np.int32), q, M) for X, ids, q, M in structs])
    assert np.array_equal(np.concatenate(z32, 0), z)
    bad = [list(s) for s in structs]
    bad[1][1] = bad[1][1].copy(); bad[1][1][0, 0] = 40      # index outside its own structure (would alias the next one)
    with pytest.raises(PestoError):
        m.forward_batch([tuple(s) for s in bad])
    assert np.array_equal(np.concatenate(m.forward_batch(structs), 0), z)


def test_sharding_forward_local_uses_device_collate():
    """pesto_amd.sharding.forward_local with a Model goes through pesto_forward_batch; results = one structure at a time,
    except that a collated batch shares one max(D) (only matters below 1e-2 A: none here) - compare within the parity bound."""
    from pesto_amd.sharding import forward_local
    from pesto_amd.topology import extract_topology, synthetic_structure
    m = _model("i_v4_0")
    structs = []
    for i, n in enumerate((300, 180, 96)):
        X, _, q, M = synthetic_structure(n, 40 + i, n0=30)
        structs.append((X, extract_topology(X, 64), q, M))
    res = forward_local(m, structs, [0, 1, 2], max_atoms=500)      # -> launches of (300), (180 + 96)
    for i, (X, ids, q, M) in enumerate(structs):
        one = m.forward_batch([(X, ids, q, M)])[0]
        assert res[i].shape == one.shape and np.abs(res[i] - one).max() < 1e-4
    zo = _oracle("i_v4_0")
    roa = structs[0][3].argmax(1).astype(np.int32)
    ref = zo.forward_segments(structs[0][0], (structs[0][1] + 1).astype(np.int32), structs[0][2], roa, structs[0][3].shape[1])
    assert np.abs(res[0] - ref).max() < 1e-4


@pytest.mark.parametrize("n", [1, 2, 3, 17, 63, 64, 65])
def test_tiny_structures_vs_oracle(n, impl):
    """Degenerate sizes: a single atom (every neighbour slot is padding -> wraps to itself, D = 0, the max(D) fix-up with
    max = 0), two or three atoms, and the N = 63 / 64 / 65 boundary of the 64-column table (self among the neighbours up to 64)."""
    from pesto_amd.topology import extract_topology, synthetic_cloud
    rng = np.random.default_rng(100 + n)
    X = synthetic_cloud(n, 100 + n)          # protein-like density, no sub-0.5 A contacts (dense random clouds are ill-conditioned:
    ids0 = extract_topology(X, 64)           # there even the exact-fp32 path and the oracle differ by 1e-4, |z| > 20)
    ids = np.zeros((n, 64), np.int64)
    ids[:, :ids0.shape[1]] = ids0 + 1
    q = np.zeros((n, 30), np.float32)
    q[np.arange(n), rng.integers(0, 5, n)] = 1.0
    roa = (np.arange(n) // 2).astype(np.int32)
    R = int(roa.max()) + 1
    z_h = _model("i_v4_0").forward_segments(X, ids, q, roa, R)
    z_o = _oracle("i_v4_0").forward_segments(X, ids, q, roa, R)
    assert np.isfinite(z_o).all() == np.isfinite(z_h).all()
    if np.isfinite(z_o).all():
        assert np.abs(z_h - z_o).max() < 1e-4
    else:                                   # N = 1: D = 0 everywhere -> 0/0 in the reference too; both sides must agree on where
        assert np.array_equal(np.isfinite(z_h), np.isfinite(z_o))


@pytest.mark.parametrize("fixture", ["fwd_i_v4_0_2CUA", "fwd_i_v4_0_2AYO"])
def test_knn_on_real_chains_matches_reference_topology(fixture):
    """GPU k-NN on real protein coordinates (2CUA: 955 atoms, 2AYO: 2,810 atoms) against the ids the reference's
    extract_topology + collate_batch_features produced for the whole-forward fixtures."""
    g = golden(fixture)
    m = _model("i_v4_0")
    ids = m.knn_collate(g["X"], [g["X"].shape[0]])
    _check_same_neighbours(ids, g["ids_topk"].astype(np.int64), g["X"])
    z = m.forward_segments(g["X"], ids, onehot(g["q_idx"], 30), g["res_of_atom"], g["z"].shape[0])
    assert np.abs(z - g["z"]).max() < 1e-4


def test_batch_equals_singles_bitwise_across_kernel_instantiations():
    """A 16.8k-atom batch runs every layer on the full-size kernels (12-wave workgroups, 4 tiles per work item); its members
    alone run on the small-launch instantiations (8 waves, 1-2 tiles per item). Same bits either way (-ffp-contract=on)."""
    from pesto_amd.topology import extract_topology, synthetic_structure
    m = _model("i_v4_0")
    structs = []
    for i in range(6):
        X, _, q, M = synthetic_structure(2800, 70 + i, n0=30)
        structs.append((X, extract_topology(X, 64), q, M))
    zb = m.forward_batch(structs)
    for i in (0, 3, 5):
        assert np.array_equal(zb[i], m.forward_batch([structs[i]])[0])


# ---------------------------------------------------------------------------------------------- k-NN cell grid (large structures)
def _knn_both_paths(m, X, sizes):
    grid = m.debug_select(0, knn_brute_force=False).knn_collate(X, sizes)
    brute = m.debug_select(0, knn_brute_force=True).knn_collate(X, sizes)
    m.debug_select(0, knn_brute_force=False)
    return grid, brute


def test_knn_cell_grid_equals_brute_force():
    """Structures of >= 1024 atoms are searched through a uniform cell grid; the table must be the brute-force one, bit for bit:
    protein-like cloud, a mixed batch (large + small members), a flat slab (one cell layer), two dense blobs far apart (most
    cells empty, blocks must grow), and atoms on a line."""
    from pesto_amd.topology import synthetic_cloud
    m = _model("i_v4_0")
    rng = np.random.default_rng(3)
    cloud = synthetic_cloud(6000, 21)
    slab = synthetic_cloud(5000, 22); slab[:, 2] *= 0.02
    blobs = np.concatenate([synthetic_cloud(2500, 23), synthetic_cloud(2500, 24) + 400.0]).astype(np.float32)
    line = np.zeros((4500, 3), np.float32); line[:, 0] = np.arange(4500) * 1.3 + rng.uniform(0, 0.3, 4500)
    for X, sizes in ((cloud, [6000]), (np.concatenate([cloud[:4200], cloud[4200:5400], cloud[5400:], slab]), [4200, 1200, 600, 5000]),
                     (slab, [5000]), (blobs, [5000]), (line, [4500]), (cloud[:1024], [1024])):
        grid, brute = _knn_both_paths(m, np.ascontiguousarray(X, np.float32), sizes)
        assert np.array_equal(grid, brute)
        assert grid.min() >= 1 and grid.max() <= X.shape[0]


def test_knn_cell_grid_vs_host_contract_and_forward():
    from pesto_amd.topology import extract_topology, synthetic_structure
    m = _model("i_v4_0")
    X, _, q, M = synthetic_structure(5000, 31, n0=30)
    ids = m.knn_collate(X, [5000])
    _check_same_neighbours(ids, extract_topology(X, 64) + 1, X)        # host contract (k-d tree above 4096 atoms)
    roa = M.argmax(1).astype(np.int32)
    z = m.forward_segments(X, ids, q, roa, M.shape[1])
    zo = _oracle("i_v4_0").forward_segments(X, ids.astype(np.int32), q, roa, M.shape[1])
    assert np.abs(z - zo).max() < 1e-4


def _knn_edge_cloud(name):
    """(X, sizes) at the edges of the shared cell grid (pesto_cellgrid.h). The seeds were chosen on the host so that in no structure of
    more than 64 atoms an exact key tie decides a column of extract_topology's table (checked by sorting once with ties broken by the
    smallest and once by the largest index), except in the two clouds of coincident atoms, where every tie is between keys that both
    sides order by index."""
    from pesto_amd.topology import synthetic_cloud
    rng = np.random.default_rng(300)
    if name in ("n1023", "n1024", "n1025"):                  # the threshold between brute force and the grid
        n = int(name[1:])
        return synthetic_cloud(n, {1023: 301, 1024: 300, 1025: 302}[n]), [n]
    if name == "batch":                                      # small members between large ones: g.base, sorted.w - s0
        sizes = [1500, 40, 1024, 7, 3000]
        return np.concatenate([synthetic_cloud(n, 300) for n in sizes]), sizes
    if name == "sparse_cube":                                # the cell cap: the edge grows by 1.25, most cells empty, the blocks must grow
        return rng.uniform(0, 250, (1024, 3)).astype(np.float32), [1024]
    if name == "line":                                       # more than 64 cells of 4.5 A along x: ext / 64 governs the edge
        X = rng.uniform(0, 0.05, (2000, 3)).astype(np.float32)
        X[:, 0] += (np.arange(2000) * 0.2).astype(np.float32)
        return X, [2000]
    if name == "coincident":                                 # masked keys among the first 64 of 1,050 rows: the blocks grow to the whole grid
        X = synthetic_cloud(1100, 320)
        X[50:] = X[50]
        return X, [1100]
    if name == "point":                                      # ... and a zero-extent box: one cell, every key masked
        return np.full((1100, 3), 3.25, np.float32), [1100]
    if name == "flat_x":                                     # one cell layer
        X = synthetic_cloud(1200, 300)
        X[:, 0] = np.float32(7.5)
        return X, [1200]
    assert name == "cloud2000"
    return synthetic_cloud(2000, 300), [2000]


@functools.lru_cache(maxsize=None)
def _knn_edge_reference(name):
    """X, sizes and the table of the host contract (extract_topology per structure, 1-based batch-global ids), computed once"""
    from pesto_amd.topology import extract_topology
    X, sizes = _knn_edge_cloud(name)
    ref = np.zeros((X.shape[0], 64), np.int64)
    off = 0
    for n in sizes:
        ref[off:off + n, :min(n, 64)] = extract_topology(X[off:off + n], 64) + off + 1
        off += n
    return X, sizes, ref


def _check_knn_edge(m, name, k=64):
    X, sizes, ref = _knn_edge_reference(name)
    grid = m.debug_select(0, knn_brute_force=False).knn_collate(X, sizes, k)
    brute = m.debug_select(0, knn_brute_force=True).knn_collate(X, sizes, k)
    m.debug_select(0, knn_brute_force=False)
    assert np.array_equal(grid, brute)
    assert not grid[:, k:].any()
    ref = ref[:, :k]
    off = 0
    for n in sizes:
        got, want = grid[off:off + n, :k], ref[off:off + n]
        _check_same_neighbours(got, want, X[off:off + n], offset=off)
        if n > 64:          # (a smaller structure lists the atom itself, whose key ties with the farthest atom's by the reference's rule)
            assert np.array_equal(got, want)
        off += n
    return grid


@pytest.mark.parametrize("name", ["n1023", "n1024", "n1025", "batch", "sparse_cube", "line", "coincident", "point", "flat_x"])
def test_knn_shared_cell_grid_edges(name):
    """The k-NN on the cell grid it shares with the contact searches: at every edge of that grid the table is the brute-force one bit for
    bit and the host contract's (extract_topology), which does not know the kernel."""
    _check_knn_edge(_model("i_v4_0"), name)


@pytest.mark.parametrize("k", [16, 1])
def test_knn_shared_cell_grid_fewer_columns(k):
    _check_knn_edge(_model("i_v4_0"), "cloud2000", k)


def test_knn_shared_cell_grid_device_input_equals_host_input():
    import torch
    m = _model("i_v4_0")
    X, sizes, _ = _knn_edge_reference("batch")
    ids = _check_knn_edge(m, "batch")
    ids_dev = m.to("cuda:0").knn_collate(torch.from_numpy(X).cuda(), sizes)
    assert ids_dev.is_cuda and torch.equal(ids_dev.cpu(), torch.from_numpy(ids))


def test_bulk_apply_model_pdb_in_pdb_out(tmp_path):
    """pesto_amd.apply.apply_model: PDB files -> probabilities + b-factor PDB files, several structures per launch, host stages in
    threads. Checked against the one-structure-at-a-time chain; an unreadable file is reported and skipped."""
    import gzip
    import os
    from conftest import GOLDEN
    from pesto_amd.apply import apply_model
    from pesto_amd.structure_io import Structure
    m = _model("i_v4_0").to("cuda")
    paths = []
    for name in ("7KHT_lipid", "1thf_D", "6I9F"):
        p = tmp_path / (name + ".pdb")
        p.write_text(gzip.open(os.path.join(GOLDEN, "pdb", name + ".pdb.gz"), "rt").read())
        paths.append(str(p))
    bad = tmp_path / "broken.pdb"
    bad.write_text("ATOM      1  N   ALA A   1      30.837\n")
    errors = []
    from pesto_amd.apply import load_results
    res = apply_model(m, paths[:2] + [str(bad)] + paths[2:], max_atoms=4500, workers=4, on_error=errors.append,
                      results_path=str(tmp_path / "bulk.npz"))
    assert set(res) == set(paths) and len(errors) == 1 and "broken.pdb" in errors[0]
    stored = load_results(str(tmp_path / "bulk.npz"))               # the bulk store (the reference's hf[key] = p)
    assert set(stored) == set(paths) and all(np.array_equal(stored[k], res[k]) for k in paths)
    from pesto_amd import h5store
    if h5store.available():                                         # ... and as the HDF5 file the reference's loop writes (no h5py: libhdf5 through ctypes)
        from pesto_amd.apply import save_results
        h5 = load_results(save_results(res, str(tmp_path / "bulk.h5")))
        assert set(h5) == {k.lstrip("/") for k in paths} and all(np.array_equal(h5[k.lstrip("/")], res[k]) for k in paths)
    for p in paths:
        s = Structure.read_pdb(p).preprocess()
        X, q, roa, R = s.encode(30)
        ids = m.knn_collate(X, [len(s)])
        z = m.forward_segments(X, ids, q, roa, R)
        pr, bf = m.postprocess(z, roa)
        assert res[p].shape == pr.shape and np.abs(res[p] - pr).max() < 1e-5
        for c in range(5):
            got = open(p[:-4] + f"_i{c}.pdb").read()
            assert got.count("\n") == s.format_pdb(bf[c]).count("\n")
            b_got = np.array([float(l[54:60]) for l in got.split("\n") if l.startswith(("ATOM", "HETATM"))])
            assert np.abs(b_got - np.round(bf[c].astype(np.float64), 2)).max() < 0.0101


def test_knn_fewer_columns_than_64():
    """k < 64: the first k columns are the k nearest, the rest of the 64-column table is zero padding (grid and brute-force paths)."""
    from pesto_amd.topology import synthetic_cloud
    m = _model("i_v4_0")
    for n in (300, 2000):
        X = synthetic_cloud(n, 77)
        full = m.knn_collate(X, [n])
        part = m.knn_collate(X, [n], k=16)
        assert np.array_equal(part[:, :16], full[:, :16]) and not part[:, 16:].any()


# ---------------------------------------------------------------------------------------------- round 2: config 4, config 3 at size, range guard
def test_config4_pdbs_test_chains_sharded_and_batched():
    """BASELINE config 4: chains of the reference's pdbs_test/ (1,641 - 3,052 atoms) through the i_v4_1 architecture against the
    reference's one-structure-per-call outputs, via sharding.forward_sharded (single process = world 1) and Model.forward_batch;
    any grouping into launches gives the same bits (PESTO_BATCH_INDEPENDENT)."""
    from pesto_amd.sharding import forward_sharded
    m = _model("i_v4_1")
    structs, refs = [], []
    for name in CFG4_CHAINS:
        X, ids0, q, M, z = cfg4_structure(name)
        structs.append((X, ids0, q, M)); refs.append(z)
    sharded = forward_sharded(m, structs, n_out=5, max_atoms=8000)          # launches of 3 + 2 chains
    one_launch = m.forward_batch(structs, independent=True)
    for i, z in enumerate(refs):
        assert sharded[i].shape == z.shape and np.abs(sharded[i] - z).max() < 1e-4, CFG4_CHAINS[i]
        assert np.array_equal(sharded[i], one_launch[i])
        assert np.array_equal(sharded[i], m.forward_batch([structs[i]], independent=True)[0])
    # the same chains as ONE collated batch with device tensors and per-structure semantics (what apply_model does)
    import torch
    from pesto_amd.topology import collate_batch_features, mask_to_segments
    X, ids, q, M = collate_batch_features([list(s) for s in structs])
    roa, R = mask_to_segments(M)
    dev = torch.device("cuda:0")
    zc = m.to(dev).forward_segments(torch.from_numpy(X).to(dev), torch.from_numpy(ids).to(dev), torch.from_numpy(q).to(dev),
                                    torch.from_numpy(roa).to(dev), R, sizes=[s[0].shape[0] for s in structs]).cpu().numpy()
    assert np.array_equal(zc, np.concatenate(one_launch, 0))


@pytest.mark.parametrize("tag,zkey,qkey", [("i_v4_1", "z", "q0"), ("i_v4_0", "z_i_v4_0", "q0"), ("i_v3_0", "z_i_v3_0", "q0_all")])
def test_config4_all_53_pdbs_test_chains(tag, zkey, qkey):
    """BASELINE config 4 IN FULL: every chain of the reference's pdbs_test/ (53 chains, 1,641 - 3,052 atoms, 132 k atoms) against the
    reference's one-structure-per-call logits (interfaceome/apply_model.py:57-82), fed the reference's own neighbour ids, through
    sharding.forward_local - the pipelined bulk path with launches packed to <= 24,576 atoms. Three models: the i_v4_1 architecture
    (32 layers, stacked weights) and the TRAINED i_v4_0 and i_v3_0 (123 input features) checkpoints. The GPU k-NN
    (pesto_knn_collate) must reproduce the host topology on every chain (which equals the reference's up to the order of exact fp32
    distance ties)."""
    from conftest import cfg4_all53
    from pesto_amd.sharding import forward_local
    m = _model(tag)
    chains = cfg4_all53()
    assert len(chains) == 53
    structs = []
    for ch in chains:
        if tag == "i_v4_1":
            ids_gpu = m.knn_collate(ch["X"], [ch["X"].shape[0]])
            assert np.array_equal(ids_gpu, ch["ids0_host"].astype(np.int64) + 1), ch["name"]
        roa = ch["res_of_atom"]
        M = np.zeros((roa.size, ch["R"]), np.float32)
        M[np.arange(roa.size), roa] = 1.0
        structs.append((ch["X"], ch["ids0"], ch[qkey], M))
    out = forward_local(m, structs, list(range(len(structs))))
    assert m.status()["n_fp32_rerun"] == 0      # these models stay inside the f16 range on real chains: no launch repeated in fp32
    worst = 0.0
    for i, ch in enumerate(chains):
        zh = out[i]
        assert zh is not None and zh.shape == ch[zkey].shape, ch["name"]
        err = float(np.abs(zh - ch[zkey]).max())
        worst = max(worst, err)
        assert err < 1e-4, (ch["name"], err)
    print(f"config 4, 53 chains, {tag}: max |hip - reference| = {worst:.2e}")


def test_drop_in_knn_path_on_all_53_chains_ties_are_reported():
    """The DROP-IN path (GPU k-NN inside, no patched ids) on all 53 pdbs_test chains: the tables differ from the reference's only on rows
    with two neighbours at exactly the same float32 distance (torch.topk's order there is undefined, src/data_encoding.py:98-99; here:
    by index). pesto_knn_tie_rows reports the rows on which such a tie STRADDLES a neighbourhood cut-off - the only rows where the
    difference can move a logit. Asserted: (1) the report equals a numpy statement of the same rule, entry for entry; (2) every row of
    the fixture's patch list (where the reference's table differs) whose swap crosses a cut is reported for that cut; (3) every chain
    whose logits deviate from the reference by more than 1e-4 has a reported row on a cut its model uses - all other chains are inside
    the bound with the GPU table as it is."""
    from conftest import cfg4_all53, golden as _g
    from pesto_amd.topology import _norm_xyz
    m = _model("i_v4_0", "mfma")
    chains = cfg4_all53()
    patches = _g("cfg4_all53")["tie_patches"]
    structs, flagged, n_rows = [], [], 0
    for ci, ch in enumerate(chains):
        X = ch["X"]
        n = X.shape[0]
        ids = m.knn_collate(X, [n])                              # 1-based
        assert np.array_equal(ids, ch["ids0_host"].astype(np.int64) + 1)
        fl = m.knn_tie_rows(X, [n], ids)
        # (1) numpy statement for this chain: distances of every atom pair as the library rounds them (FMA-chain norm)
        if ci % 9 == 0:
            D = _norm_xyz(X[None, :, :] - X[:, None, :])       # [i, j]
            key = np.where(D < 1e-2, D + 1e9, D)                # masked entries sort behind every other atom, by D among themselves
            np.fill_diagonal(key, -1.0)                        # the atom itself is no candidate on either side (round 5)
            want = np.zeros(n, np.uint8)
            for c, cut in enumerate((8, 16, 32, 64)):
                kc = key[np.arange(n), ids[:, cut - 1] - 1]
                inside = (key[np.arange(n)[:, None], ids[:, :cut] - 1] == kc[:, None]).sum(1)
                want |= ((key == kc[:, None]).sum(1) > inside).astype(np.uint8) << c
            assert np.array_equal(fl, want), ch["name"]
        # (2) the fixture's patch rows: a swap of slots (c - 1, c) with c a cut must be reported for that cut
        rows = patches[patches[:, 0] == ci]
        for r in np.unique(rows[:, 1]):
            cols = sorted(int(v) for v in rows[rows[:, 1] == r][:, 2])
            for b, cut in enumerate((8, 16, 32)):
                if cut - 1 in cols and cut in cols:
                    assert fl[r] & (1 << b), (ch["name"], int(r), cut)
        flagged.append(fl)
        n_rows += int((fl != 0).sum())
        roa = ch["res_of_atom"]
        M = np.zeros((roa.size, ch["R"]), np.float32)
        M[np.arange(roa.size), roa] = 1.0
        structs.append((X, (ids - 1).astype(np.int32), ch["q0"], M))
    from pesto_amd.sharding import forward_local
    out = forward_local(m, structs, list(range(len(structs))))
    n_dev = 0
    for ci, ch in enumerate(chains):
        err = float(np.abs(out[ci] - ch["z_i_v4_0"]).max())
        if err >= 1e-4:
            n_dev += 1
            assert (flagged[ci] & 0x0f).any(), (ch["name"], err)      # i_v4_0 uses nn = 8, 16, 32 and 64 (k = 64: the 64 / 65 tie changes the SET)
    print(f"\n   drop-in k-NN path, 53 chains: {n_rows} of 132,417 rows reported (a tie straddles a cut), {n_dev} chain(s) beyond 1e-4, all of them reported")
    assert n_rows < 200 and n_dev <= 3


@pytest.mark.parametrize("tag,zkey,qkey", [("i_v4_0", "z_i_v4_0", "q0"), ("i_v3_0", "z_i_v3_0", "q0_all")])
def test_example_complexes_with_nucleic_acids_lipids_ions(tag, zkey, qkey):
    """Seven multi-chain complexes of the reference's examples/ (DNA / RNA, lipids, ions, ligands next to protein chains; 955 - 15,635
    atoms, i.e. also beyond the sizes where the host topology uses its k-d tree and the GPU k-NN its cell grid) through the TRAINED
    i_v4_0 / i_v3_0 checkpoints against the reference's logits (apply_model.ipynb cell 6: read, preprocess, encode, topology,
    forward). One launch for all of them; the GPU k-NN must reproduce the host topology."""
    from conftest import example_complexes
    m = _model(tag)
    cx = example_complexes()
    assert len(cx) == 7
    structs = []
    for ch in cx:
        if tag == "i_v4_0":
            assert np.array_equal(m.knn_collate(ch["X"], [ch["X"].shape[0]]), ch["ids0_host"].astype(np.int64) + 1), ch["name"]
        roa = ch["res_of_atom"]
        M = np.zeros((roa.size, ch["R"]), np.float32)
        M[np.arange(roa.size), roa] = 1.0
        structs.append((ch["X"], ch["ids0"], ch[qkey], M))
    out = m.forward_batch(structs, independent=True)
    assert m.status()["n_fp32_rerun"] == 0
    for ch, zh in zip(cx, out):
        assert zh.shape == ch[zkey].shape, ch["name"]
        assert np.abs(zh - ch[zkey]).max() < 1e-4, (ch["name"], float(np.abs(zh - ch[zkey]).max()))


def test_config3_i_v3_0_at_n3000():
    """BASELINE config 3 at its stated size (i_v3_0: 16 layers, 123 input features, real weights; synthetic N=3000)."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    gs = golden("fwd_i_v3_0_synth3000")
    X, ids0, q, M = synthetic_structure(3000, int(gs["seed"]), n0=123)
    roa, R = mask_to_segments(M)
    z = _model("i_v3_0").forward_segments(X, ids0 + 1, q, roa, R)
    assert np.abs(z - gs["z"]).max() < 1e-4


def test_softmax_range_is_guarded_not_assumed():
    """The split kernels evaluate the attention softmax (src/model_operations.py:139-140) as exp2(t) / sum exp2(t) WITHOUT torch's max
    subtraction: the same function while the logits stay inside the fp32 exponent range (trained checkpoints: -39 .. +64,
    profiles/r05_logit_range.txt). Outside it the result must never be a plausible wrong number: a centre whose sum overflows or whose
    every term underflows trips the range guard of its structure - "auto" repeats it on the exact kernels (max-subtracted), "f16_split"
    fails loudly. Logits are scaled through the last nqm layer of the first state-update layer (Q = nqm(X_n), :119)."""
    from oracle import oracle
    from pesto_amd import Model
    from pesto_amd._lib import ERR_RANGE, PestoError
    g = golden("fwd_i_v4_0_2CUA")
    roa = g["res_of_atom"]
    args = (g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)

    def scaled(f):
        sd = dict(weights("i_v4_0"))
        for k in ("sum.0.su.nqm.4.weight", "sum.0.su.nqm.4.bias"):
            sd[k] = (np.asarray(sd[k]) * np.float32(f)).astype(np.float32)
        return sd
    # x4: sharper softmaxes, still far inside the exponent range: no repeat, and the unsubtracted form agrees with the max-subtracted oracle
    sd4 = scaled(4.0)
    m = Model(CONFIGS["i_v4_0"]); m.load_state_dict(sd4)
    z4 = m.forward_segments(*args)
    assert m.status()["n_fp32_rerun"] == 0
    z4_ref = oracle.OracleModel(CONFIGS["i_v4_0"], sd4, wide=True).forward_segments(args[0], args[1], args[2], roa, args[4])
    assert np.abs(z4 - z4_ref).max() < 1e-4, np.abs(z4 - z4_ref).max()
    # x400: logits of several hundred - exp2 overflows (or every term of a row flushes): flagged, repeated, equal to the exact kernels
    sd400 = scaled(400.0)
    m = Model(CONFIGS["i_v4_0"]); m.load_state_dict(sd400)
    z_auto = m.forward_segments(*args)
    assert np.isfinite(z_auto).all() and m.status()["n_fp32_rerun"] == 1
    z_fp32 = m.set_precision("fp32").forward_segments(*args)
    assert np.array_equal(z_auto, z_fp32)
    z_ref = oracle.OracleModel(CONFIGS["i_v4_0"], sd400, wide=True).forward_segments(args[0], args[1], args[2], roa, args[4])
    assert np.abs(z_auto - z_ref).max() < 1e-3, np.abs(z_auto - z_ref).max()      # (saturated softmaxes: near-ties cost more than 1e-4)
    m.set_precision("f16_split")
    with pytest.raises(PestoError) as e:
        m.forward_segments(*args)
    assert e.value.code == ERR_RANGE


def test_auto_says_once_when_it_repeats_every_structure(caplog):
    """under the default policy the trained i_v3_1 pays the split AND the exact kernels on every structure (its states
    leave the f16 range). pesto_get_auto_counters counts structures forwarded / repeated; the Python layer logs ONE warning pointing at
    precision="fp32" once at least 90 % of >= 16 structures were repeated - and nothing for a model that never repeats."""
    import logging
    from pesto_amd import Model
    g = golden("fwd_i_v3_0_2CUA")
    roa = g["res_of_atom"]
    args = (g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 123), roa, int(roa.max()) + 1)
    m = Model(CONFIGS["i_v3_1"])
    m.load_state_dict(weights("i_v3_1_trained"))
    with caplog.at_level(logging.WARNING, logger="pesto_amd"):
        for _ in range(15):
            m.forward_segments(*args)
        assert m.auto_counters() == {"n_structures": 15, "n_repeated": 15} and not caplog.records
        for _ in range(20):
            m.forward_segments(*args)
        hits = [r for r in caplog.records if "precision='fp32'" in r.getMessage()]
        assert len(hits) == 1 and "repeated 16 of 16" in hits[0].getMessage()
    ok = _model("i_v3_0", "mfma")
    with caplog.at_level(logging.WARNING, logger="pesto_amd"):
        caplog.clear()
        for _ in range(33):
            ok.forward_segments(*args)
        assert ok.auto_counters() == {"n_structures": 33, "n_repeated": 0} and not caplog.records
    m.set_precision("fp32")
    m.forward_segments(*args)
    assert m.auto_counters()["n_structures"] == 35      # (fp32 forwards are not "auto" structures)


def test_trained_i_v3_1_range_guard():
    """The reference's TRAINED i_v3_1 drives its states to 4e5, beyond the f16 range of the split-MFMA kernels. "auto" must notice
    and compute the structure again on the exact fp32 kernels (finite, within the reference's own fp32-vs-fp64 noise) - before the
    call returns, also with device tensors; with async_auto the check is deferred to the next call on the handle. "f16_split" must
    fail loudly (error on the synchronising path, NaN logits on the asynchronous one) - never a plausible wrong number."""
    import torch
    from pesto_amd import Model
    from pesto_amd._lib import ERR_RANGE, PestoError
    from test_oracle import i_v3_1_bound
    g, ref = golden("fwd_i_v3_0_2CUA"), golden("fwd_i_v3_1_2CUA")
    roa = g["res_of_atom"]
    args = (g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 123), roa, int(roa.max()) + 1)
    m = Model(CONFIGS["i_v3_1"])                                   # precision "auto" is the default
    m.load_state_dict(weights("i_v3_1_trained"))
    z_auto = m.forward_segments(*args)
    st = m.status()
    assert st["precision"] == "auto" and st["n_fp32_rerun"] == 1 and st["n_forward"] == 2
    assert z_auto.shape == ref["z"].shape and i_v3_1_bound(z_auto, ref)
    m.set_precision("fp32")
    z_fp32 = m.forward_segments(*args)
    assert np.array_equal(z_fp32, z_auto) and m.status()["n_fp32_rerun"] == 1
    # no history: "auto" tries the split kernels on every call (a structure's bits must not depend on what the handle saw before)
    assert np.array_equal(m.set_precision("auto").forward_segments(*args), z_auto) and m.status()["n_fp32_rerun"] == 2
    assert np.array_equal(m.forward_segments(*args), z_auto) and m.status()["n_fp32_rerun"] == 3
    # device tensors: checked (and repeated) before the call returns - a drop-in caller can go on with torch.sigmoid(z)
    dev = torch.device("cuda:0")
    m.to(dev)
    targs = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in args[:4]]
    z_dev = m.forward_segments(*targs, args[4])
    assert np.array_equal(z_dev.cpu().numpy(), z_auto) and m.status()["n_fp32_rerun"] == 4
    zf_dev = m.forward_frames_segments(torch.stack([targs[0], targs[0]]), *targs[1:4], args[4])     # the frames path too
    assert np.array_equal(zf_dev[0].cpu().numpy(), z_auto) and np.array_equal(zf_dev[1].cpu().numpy(), z_auto) and m.status()["n_fp32_rerun"] == 6
    # async_auto: the launch returns at once; until the next call on the handle an overflowed structure holds NaN, afterwards the fp32 result
    m.set_async_auto(True)
    z_late = m.forward_segments(*targs, args[4])
    torch.cuda.synchronize()
    assert torch.isnan(z_late).all()                               # loud until the deferred check has run
    m.synchronize()
    assert np.array_equal(z_late.cpu().numpy(), z_auto) and m.status()["n_fp32_rerun"] == 7
    zf_late = m.forward_frames_segments(torch.stack([targs[0], targs[0]]), *targs[1:4], args[4])
    m.synchronize()
    assert np.array_equal(zf_late[1].cpu().numpy(), z_auto) and m.status()["n_fp32_rerun"] == 9
    m.set_async_auto(False)
    # f16_split: loud failure
    m.set_precision("f16_split")
    with pytest.raises(PestoError) as e:
        m.forward_segments(*args)
    assert e.value.code == ERR_RANGE
    z_nan = m.forward_segments(*targs, args[4])                    # asynchronous and unchecked: every logit of the structure NaN
    assert torch.isnan(z_nan).all()
    # the handle is not poisoned: a well-behaved model state afterwards
    m.set_precision("auto")
    assert np.array_equal(m.to("cpu").forward_segments(*args), z_auto)
    # bad inputs: reported by the call itself; on the asynchronous path by the next call
    m40d = _model("i_v4_0", "mfma").to(dev)
    g40 = golden("fwd_i_v4_0_2CUA")
    t40 = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (g40["X"], g40["ids_topk"].astype(np.int64), onehot(g40["q_idx"], 30), g40["res_of_atom"])]
    z_ok = m40d.forward_segments(*t40, g40["z"].shape[0])
    bad_ids = t40[1].clone(); bad_ids[5, 3] = 10 ** 6
    with pytest.raises(PestoError):
        m40d.forward_segments(t40[0], bad_ids, t40[2], t40[3], g40["z"].shape[0])
    m40d.set_async_auto(True)
    z_bad = m40d.forward_segments(t40[0], bad_ids, t40[2], t40[3], g40["z"].shape[0])             # returns at once
    with pytest.raises(PestoError):
        m40d.synchronize()
    assert torch.isnan(z_bad).all()
    assert torch.equal(m40d.forward_segments(*t40, g40["z"].shape[0]), z_ok)
    # and a model that stays in range never pays for the guard
    m40 = _model("i_v4_0", "mfma")
    m40.forward_segments(g40["X"], g40["ids_topk"], onehot(g40["q_idx"], 30), g40["res_of_atom"], g40["z"].shape[0])
    assert m40.status() == {"precision": "auto", "n_forward": 1, "n_fp32_rerun": 0}


def _exploded(st, factor=3.0e4):
    """the same structure with coordinates scaled so that its distances (1e5) leave the f16 range inside the first edge layer"""
    return (st[0] * np.float32(factor),) + tuple(st[1:])


def test_range_guard_is_per_structure():
    """SURVEY 8e acceptance under the DEFAULT precision: a structure's bits do not depend on its batch mates, also when one of them
    leaves the f16 range. A launch of [clean, overflowing, clean, overflowing, clean (N < 64)] through the trained i_v4_0: only the two
    flagged members are computed again on the fp32 kernels (n_fp32_rerun counts structures); every member equals its own call bit for
    bit - the clean ones on the split kernels, the flagged ones on the exact kernels - on the synchronous batch call, the pipelined
    submit / wait path, the collated device call with structure offsets, and as trajectory frames (the guard is per frame)."""
    import torch
    from pesto_amd.topology import collate_batch_features, mask_to_segments
    m = _model("i_v4_0", "mfma")
    parts = _split_batch_fixture(golden("edge_batch2"))           # 300 + 40 atoms
    g = golden("fwd_i_v4_0_2CUA")
    roa = g["res_of_atom"]
    Mc = np.zeros((roa.size, int(roa.max()) + 1), np.float32); Mc[np.arange(roa.size), roa] = 1
    big = (g["X"], g["ids_topk"].astype(np.int32) - 1, onehot(g["q_idx"], 30), Mc)      # 955 atoms
    structs = [parts[0], _exploded(big), big, _exploded(parts[0]), parts[1]]
    flagged = [False, True, False, True, False]
    solo = []
    for st, f in zip(structs, flagged):
        n0 = m.status()["n_fp32_rerun"]
        solo.append(m.forward_batch([st], independent=True)[0])
        assert m.status()["n_fp32_rerun"] == n0 + (1 if f else 0)
        assert np.isfinite(solo[-1]).all()
    m.set_precision("fp32")
    for st, f, z in zip(structs, flagged, solo):
        if f:
            assert np.array_equal(m.forward_batch([st], independent=True)[0], z)      # a flagged structure = its exact-kernel result
    m.set_precision("f16_split")
    for st, f, z in zip(structs, flagged, solo):
        if not f:
            assert np.array_equal(m.forward_batch([st], independent=True)[0], z)      # a clean one = its split-kernel result
    m.set_precision("auto")
    n0 = m.status()["n_fp32_rerun"]
    zb = m.forward_batch(structs, independent=True)
    assert m.status()["n_fp32_rerun"] == n0 + 2
    zp = m.forward_batch_wait(m.forward_batch_submit(structs, independent=True))
    assert m.status()["n_fp32_rerun"] == n0 + 4
    for j in range(len(structs)):
        assert np.array_equal(zb[j], solo[j]) and np.array_equal(zp[j], solo[j]), j
    # f16_split: only the flagged members are NaN on the asynchronous device path; the others keep their logits
    dev = torch.device("cuda:0")
    Xc, idc, qc, Mcol = collate_batch_features([list(s) for s in structs])
    roa_c, R_c = mask_to_segments(Mcol)
    sizes = [s[0].shape[0] for s in structs]
    roffs = np.cumsum([0] + [s[3].shape[1] for s in structs])
    md = _model("i_v4_0", "mfma").to(dev)
    t = [torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (Xc, idc.astype(np.int64), qc, roa_c)]
    zd = md.forward_segments(*t, R_c, sizes=sizes).cpu().numpy()            # "auto", device pointers: final at return
    for j in range(len(structs)):
        assert np.array_equal(zd[roffs[j]:roffs[j + 1]], solo[j]), j
    assert md.status()["n_fp32_rerun"] == 2
    md.set_precision("f16_split")
    zs = md.forward_segments(*t, R_c, sizes=sizes).cpu().numpy()
    for j, f in enumerate(flagged):
        blk = zs[roffs[j]:roffs[j + 1]]
        assert np.isnan(blk).all() if f else np.array_equal(blk, solo[j]), j
    # trajectory frames: frame 1 of 3 exploded - the guard and the repeat are per frame
    md.set_precision("auto")
    n0 = md.status()["n_fp32_rerun"]
    Xf = np.stack([big[0], big[0] * np.float32(3.0e4), big[0]])
    zf = md.forward_frames_segments(torch.from_numpy(Xf).to(dev), torch.from_numpy(g["ids_topk"].astype(np.int64)).to(dev),
                                    torch.from_numpy(big[2]).to(dev), torch.from_numpy(roa.astype(np.int32)).to(dev), int(roa.max()) + 1).cpu().numpy()
    assert md.status()["n_fp32_rerun"] == n0 + 1
    assert np.array_equal(zf[0], solo[2]) and np.array_equal(zf[2], solo[2]) and np.array_equal(zf[1], solo[1])


def test_range_guard_on_the_pipelined_bulk_path():
    """The TRAINED i_v3_1 (states beyond the f16 range) through pesto_forward_batch_submit / _wait with two launches in flight: under
    "auto" the flagged structures of a slot are computed again on the exact fp32 kernels from the slot's own staged inputs when it is
    waited for (the second slot was queued on the split kernels before the first one was looked at, and has used the shared workspace
    in between); "f16_split" reports PESTO_ERR_RANGE at the wait. Results = the synchronous "fp32" forward, bit for bit."""
    from pesto_amd._lib import ERR_RANGE, PestoError
    g = golden("fwd_i_v3_0_2CUA")
    roa = g["res_of_atom"]
    M = np.zeros((roa.size, int(roa.max()) + 1), np.float32)
    M[np.arange(roa.size), roa] = 1.0
    st = (g["X"], g["ids_topk"].astype(np.int32) - 1, onehot(g["q_idx"], 123), M)
    from pesto_amd import Model
    m = Model(CONFIGS["i_v3_1"])
    m.load_state_dict(weights("i_v3_1_trained"))
    z_fp32 = m.set_precision("fp32").forward_batch([st], independent=True)[0]
    assert np.isfinite(z_fp32).all()
    m.set_precision("auto")
    n0 = m.status()["n_fp32_rerun"]
    t1 = m.forward_batch_submit([st])
    t2 = m.forward_batch_submit([st, st])
    z1 = m.forward_batch_wait(t1)
    z2 = m.forward_batch_wait(t2)
    assert np.array_equal(z1[0], z_fp32) and np.array_equal(z2[0], z_fp32) and np.array_equal(z2[1], z_fp32)
    assert m.status()["n_fp32_rerun"] == n0 + 3                       # structures, not launches
    z3 = m.forward_batch_wait(m.forward_batch_submit([st]))          # no history: tried on the split kernels again, repeated again
    assert np.array_equal(z3[0], z_fp32) and m.status()["n_fp32_rerun"] == n0 + 4
    m.set_precision("f16_split")
    t = m.forward_batch_submit([st])
    with pytest.raises(PestoError) as e:
        m.forward_batch_wait(t)
    assert e.value.code == ERR_RANGE
    assert np.array_equal(m.set_precision("auto").forward_batch([st], independent=True)[0], z_fp32)      # the handle still works


def test_forward_batch_independent_equals_one_call_per_structure():
    """PESTO_BATCH_INDEPENDENT: structures with fewer than 64 atoms (zero-padded neighbour slots wrap to the structure's OWN last
    atom) and with coincident atoms (max(D) of the structure, not of the batch) get exactly the result of their own call,
    whatever they are batched with; PESTO_BATCH_COLLATED reproduces the reference's collated forward instead (edge_batch2)."""
    from pesto_amd.topology import extract_topology, synthetic_structure
    m = _model("i_v4_0")
    structs = _split_batch_fixture(golden("edge_batch2"))           # 300 + 40 atoms
    g = golden("edge_coincident")                                    # 150 atoms, D < 1e-2 entries inside the table
    roa = g["res_of_atom"]
    Mc = np.zeros((roa.size, int(roa.max()) + 1), np.float32); Mc[np.arange(roa.size), roa] = 1
    structs.append((g["X"], g["ids_topk"].astype(np.int32) - 1, onehot(g["q_idx"], 30), Mc))
    X, _, q, M = synthetic_structure(17, 3)
    structs.append((X, extract_topology(X, 64), q, M))
    singles = [m.forward_batch([s])[0] for s in structs]
    for order in ((0, 1, 2, 3), (3, 2, 1, 0), (1, 3, 0, 2)):
        zb = m.forward_batch([structs[i] for i in order], independent=True)
        for pos, i in enumerate(order):
            assert np.array_equal(zb[pos], singles[i]), (order, i)
    assert np.abs(singles[2] - g["z"]).max() < 1e-4                # a structure alone = the reference's own call
    collated = m.forward_batch(structs)
    assert not np.array_equal(collated[1], singles[1])              # the reference's batch coupling (N = 40 wraps to the batch's last atom)
    assert np.array_equal(collated[0], singles[0])


def test_calls_on_different_streams_share_the_workspace_safely():
    """One handle = one workspace. A forward queued on a torch side stream, a host-pointer call (the model's own stream) and a
    forward on the default stream, issued back to back without synchronising in between, must not overwrite each other."""
    import torch
    g = golden("fwd_i_v4_0_2AYO")
    g2 = golden("fwd_i_v4_0_2CUA")
    m = _model("i_v4_0", "mfma").set_precision("f16_split")          # asynchronous device-pointer calls
    dev = torch.device("cuda:0")
    m.to(dev)
    a = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 30), g["res_of_atom"])]
    b = [torch.from_numpy(np.ascontiguousarray(v)).to(dev) for v in (g2["X"], g2["ids_topk"].astype(np.int64), onehot(g2["q_idx"], 30), g2["res_of_atom"])]
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    for _ in range(3):
        with torch.cuda.stream(side):
            z_side = m.forward_segments(*a, g["z"].shape[0])
        z_host = m.forward_segments(g2["X"], g2["ids_topk"], onehot(g2["q_idx"], 30), g2["res_of_atom"], g2["z"].shape[0])
        z_def = m.forward_segments(*b, g2["z"].shape[0])
        with torch.cuda.stream(side):
            z_side2 = m.forward_segments(*a, g["z"].shape[0])
        torch.cuda.synchronize()
        assert np.abs(z_side.cpu().numpy() - g["z"]).max() < 1e-4 and torch.equal(z_side, z_side2)
        assert np.abs(z_host - g2["z"]).max() < 1e-4 and np.array_equal(z_def.cpu().numpy(), z_host)


# ---------------------------------------------------------------------------------------------- both work decompositions of the layer kernel
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("layer", [0, 4, 8, 12])
def test_stage_layer_forced_edge_mode(layer, mode):
    """One layer of every nn (8, 16, 32, 64) through the rendezvous mode (1) and the node-wave mode (2) of the shipped path
    (pesto_debug_edge_mode; by default chosen per launch) against the reference's per-layer goldens."""
    g = golden("ops_i_v4_0_crop200")
    m = _model("i_v4_0", "mfma").debug_edge_mode(mode)
    m.stage_unpack(g["X"], g["ids_topk"].astype(np.int32))
    q, p = m.stage_layer(layer, g[f"L{layer}_q_in"], g[f"L{layer}_p_in"])
    assert np.abs(q - g[f"L{layer}_q_out"]).max() < stage_tol(g[f"L{layer}_q_out"])
    assert np.abs(p - g[f"L{layer}_p_out"]).max() < stage_tol(g[f"L{layer}_p_out"])
    assert np.all(q[0] == 0) and np.all(p[0] == 0)


@pytest.mark.parametrize("fixture", ["fwd_i_v4_0_2AYO", "edge_n40", "edge_coincident"])
def test_forward_golden_forced_edge_modes_agree_bitwise(fixture):
    """Whole forward in each forced mode against the reference golden: 1 rendezvous, 2 node waves (the same arithmetic in the same
    order: bit-identical)."""
    g = golden(fixture)
    roa = g["res_of_atom"]
    zs = []
    for mode in (1, 2):
        m = _model("i_v4_0", "mfma").debug_edge_mode(mode)
        z = m.forward_segments(g["X"], g["ids_topk"].astype(np.int64), onehot(g["q_idx"], 30), roa, int(roa.max()) + 1)
        assert np.abs(z - g["z"]).max() < 1e-4
        zs.append(z)
    assert np.array_equal(zs[0], zs[1])      # modes 1 and 2: the same arithmetic in the same order


@pytest.mark.parametrize("atoms,batch", [(1025, 9), (6145, 2)])
def test_odd_launch_shapes_both_modes_vs_oracle(atoms, batch):
    """Launch shapes that leave partly filled rounds (9 x 1,025 atoms: one over a round multiple per structure; 2 x 6,145: one atom
    over the 6,144-atom round of the twelve-wave kernels) through both modes: against the CPU ORACLE on the same inputs, each mode
    deterministic, modes bit-identical, and batch == one call per structure bit for bit."""
    from pesto_amd.topology import mask_to_segments, synthetic_structure
    structs = [synthetic_structure(atoms, 11 * b + atoms, n0=30) for b in range(batch)]
    o = _oracle("i_v4_0")
    ref = []
    for X, ids0, q, M in structs[:2]:
        roa, R = mask_to_segments(M)
        ref.append(o.forward_segments(X, (ids0 + 1).astype(np.int32), q, roa, R))
    out = {}
    for mode in (1, 2):
        m = _model("i_v4_0", "mfma").debug_edge_mode(mode)
        zb = m.forward_batch(structs, independent=True)
        assert all(np.array_equal(a, b) for a, b in zip(zb, m.forward_batch(structs, independent=True)))
        for i in range(2):
            assert np.abs(zb[i] - ref[i]).max() < 1e-4
        for i in (0, batch - 1):
            assert np.array_equal(zb[i], m.forward_batch([structs[i]], independent=True)[0])
        out[mode] = zb
    assert all(np.array_equal(a, b) for a, b in zip(out[1], out[2]))


# ---------------------------------------------------------------------------------------------- dense mask -> segments on the GPU
def test_mask_to_segments_kernel_and_the_reference_signature():
    """Model.forward(X, ids_topk, q, M) with the dense mask ON THE DEVICE (model/model.py:32): M is reduced to res_of_atom by
    k_mask_to_segments (no ATen kernel on the path); odd R (row starts not 16-byte aligned) and aligned R; a row with two members,
    an all-zero row and an empty residue column are rejected through the forward's residue-column check."""
    import ctypes

    import torch
    from pesto_amd import _lib
    from pesto_amd._lib import PestoError
    dev = torch.device("cuda:0")
    g = golden("fwd_i_v4_0_2CUA")
    roa = g["res_of_atom"].astype(np.int64)
    R = int(roa.max()) + 1
    m = _model("i_v4_0", "mfma").to(dev)
    for pad in (0, 1, 2, 3):                      # R + pad columns: the extra residues get one atom each of a trailing dummy block
        Rp = R + pad
        N = roa.size
        M = np.zeros((N, Rp), np.float32)
        M[np.arange(N), roa] = 1.0
        if pad:
            continue_rows = np.zeros((pad, Rp), np.float32)
            continue_rows[np.arange(pad), R + np.arange(pad)] = 1.0
            Mfull = np.concatenate([M, continue_rows])
        else:
            Mfull = M
        Md = torch.from_numpy(Mfull).to(dev)
        seg, Rk = m._segments(Md)
        assert Rk == Rp and seg.dtype == torch.int32
        assert np.array_equal(seg.cpu().numpy(), Mfull.argmax(1))
    M = np.zeros((roa.size, R), np.float32)
    M[np.arange(roa.size), roa] = 1.0
    args = [torch.from_numpy(g["X"]).to(dev), torch.from_numpy(g["ids_topk"].astype(np.int64)).to(dev),
            torch.from_numpy(onehot(g["q_idx"], 30)).to(dev)]
    z = m(*args, torch.from_numpy(M).to(dev))
    assert (z.cpu() - torch.from_numpy(g["z"])).abs().max() < 1e-4
    for kind in ("two_members", "no_member", "empty_column"):
        Mb = M.copy()
        if kind == "two_members":
            Mb[7, (roa[7] + 1) % R] = 1.0
        elif kind == "no_member":
            Mb[11] = 0.0
        else:
            r = int(roa[5])
            rows = np.where(roa == r)[0]
            Mb[rows] = 0.0
            Mb[rows, (r + 1) % R] = 1.0
        with pytest.raises(PestoError):                       # precision "auto": the call checks its inputs before it returns
            m(*args, torch.from_numpy(Mb).to(dev))
        m.set_async_auto(True)
        z_bad = m(*args, torch.from_numpy(Mb).to(dev))        # asynchronous: NaN logits now, the error at the next call on the handle
        with pytest.raises(PestoError):
            m.synchronize()
        assert torch.isnan(z_bad).all()
        m.set_async_auto(False)
    # host-pointer form reports the bad row itself
    lib = _lib.load()
    Mb = M.copy(); Mb[11] = 0.0
    out = np.empty(roa.size, np.int32)
    rc = lib.pesto_mask_to_segments(m.handle, roa.size, R, Mb.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), _lib.PTR_HOST, None)
    assert rc == -1 and b"atom 11" in lib.pesto_last_error()
    rc = lib.pesto_mask_to_segments(m.handle, roa.size, R, M.ctypes.data_as(ctypes.c_void_p), out.ctypes.data_as(ctypes.c_void_p), _lib.PTR_HOST, None)
    assert rc == 0 and np.array_equal(out, roa)


# ---------------------------------------------------------------------------------------------- pipelined launches (submit / wait)
def test_forward_batch_submit_wait_equals_forward_batch_bitwise():
    """pesto_forward_batch_submit / _wait: two launches in flight, the compact input forms (uint16 neighbour ids, byte feature
    indices expanded on the GPU) and the plain ones - every structure must come back with the bits of pesto_forward_batch; a bad
    structure is reported by the wait of ITS ticket and the handle survives."""
    from pesto_amd._lib import PestoError
    from pesto_amd.topology import synthetic_structure
    m = _model("i_v4_0", "mfma")
    groups = [[synthetic_structure(n, 500 + 10 * g + i, n0=30) for i, n in enumerate(sizes)] for g, sizes in enumerate(((700, 90, 300), (40, 1200), (64, 65, 500)))]
    ref = [m.forward_batch(g, independent=True) for g in groups]
    for compact in (True, False):
        t0 = m.forward_batch_submit(groups[0], compact=compact)
        t1 = m.forward_batch_submit(groups[1], compact=compact)          # second launch queued while the first runs
        with pytest.raises(PestoError):
            m.forward_batch_submit(groups[2], compact=compact)           # both slots in flight
        z0 = m.forward_batch_wait(t0)
        t2 = m.forward_batch_submit(groups[2], compact=compact)
        z1, z2 = m.forward_batch_wait(t1), m.forward_batch_wait(t2)
        for got, want in zip((z0, z1, z2), ref):
            assert len(got) == len(want) and all(np.array_equal(a, b) for a, b in zip(got, want))
    # i_v3_0: three one-hot blocks (30 + 29 + 64 features) through the byte-index form
    m3 = _model("i_v3_0", "mfma")
    g3 = [synthetic_structure(n, 900 + n, n0=123) for n in (300, 150)]
    want = m3.forward_batch(g3, independent=True)
    got = m3.forward_batch_wait(m3.forward_batch_submit(g3))
    assert all(np.array_equal(a, b) for a, b in zip(got, want))
    # a bad neighbour index: the error belongs to that ticket, the other launch and the handle are unaffected
    bad = [list(s) for s in groups[1]]
    bad[0][1] = bad[0][1].copy(); bad[0][1][3, 2] = 4000
    tb = m.forward_batch_submit([tuple(s) for s in bad])
    tg = m.forward_batch_submit(groups[0])
    with pytest.raises(PestoError):
        m.forward_batch_wait(tb)
    assert all(np.array_equal(a, b) for a, b in zip(m.forward_batch_wait(tg), ref[0]))
    with pytest.raises(ValueError):
        m.forward_batch_wait(tg)                                         # already collected


def test_sharding_forward_local_pipelined_equals_one_call_per_structure():
    from pesto_amd.sharding import forward_local
    from pesto_amd.topology import synthetic_structure
    m = _model("i_v4_0", "mfma")
    structs = [synthetic_structure(n, 640 + i, n0=30) for i, n in enumerate((300, 180, 96, 700, 64, 1500, 20))]
    res = forward_local(m, structs, list(range(len(structs))), max_atoms=800)       # several launches, two in flight
    for i, st in enumerate(structs):
        assert np.array_equal(res[i], m.forward_batch([st], independent=True)[0])
