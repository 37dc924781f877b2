"""bench.py's bookkeeping (no GPU): the algorithmic FLOP / byte figures are SURVEY 8d's, the config-4 size histogram is the one
captured from the reference's pdbs_test/, launch packing stays within the round size, the traffic stamp tracks the kernel sources."""
import json
import os


import bench
from conftest import ROOT, golden
from pesto_amd.config import CONFIGS


def test_survey_8d_figures():
    # FLOP(n) = 2 (13,696 + 36,376 n); B(n) = 1,024 + 532 n  per atom-layer
    assert [bench.layer_flops_per_atom(n) for n in (8, 16, 32, 64)] == [609408.0, 1191424.0, 2355456.0, 4683520.0]
    assert [bench.layer_gather_bytes_per_atom(n) for n in (8, 16, 32, 64)] == [5280.0, 9536.0, 18048.0, 35072.0]
    cfg = CONFIGS["i_v4_1"]
    assert abs(sum(bench.layer_flops_per_atom(l["nn"]) for l in cfg["sum"]) - 70.72e6) < 0.01e6        # 70.72 MFLOP per atom
    assert sum(bench.layer_gather_bytes_per_atom(l["nn"]) for l in cfg["sum"]) == 543488.0              # 543,488 B per atom
    # executed MFMA work of the shipped kernels: 99 MFMAs per 16-edge tile (8 fp32 K=4 + 90 f16 K=32) + 60 per 16 centres
    per_tile = (8 * 1024 + 90 * 8192) * 2.0
    assert bench.edge_mfma_flops_per_atom(64) == 4 * per_tile + 60 * 8192 * 2.0 / 16.0
    assert bench.executed_mfma_flops(cfg, 16) > 0


def test_config4_histogram_is_the_reference_set():
    g = golden("pdbs_test_sizes")
    assert sorted(int(v) for v in g["atoms"]) == sorted(bench.PDBS_TEST_ATOMS)
    assert len(bench.PDBS_TEST_ATOMS) == 53 and sum(bench.PDBS_TEST_ATOMS) == 132417
    from pesto_amd import sharding
    sizes = [bench.PDBS_TEST_ATOMS[i % 53] for i in range(64)]
    groups = sharding.batches(list(range(64)), sizes, 24576)
    assert all(sum(sizes[i] for i in grp) <= 24576 for grp in groups) and len(groups) == 7   # 154,518 atoms: 6.3 launches' worth
    parts = sharding.partition(sizes, 8)
    loads = [sum(sizes[i] for i in p) for p in parts]
    assert max(loads) - min(loads) < 1641 and all(len(p) == 8 for p in parts)                # 8 GPUs: balanced to one small chain


def test_per_nn_table_and_rocprof_fraction():
    """bench.py's per-kernel table: every layer kernel of the forward with its def-A fraction by HIP events and - only when the committed
    profile carries the source hash of the build - by the rocprofv3 trace, its HBM-side traffic and traffic / compulsory bytes."""
    cfg = CONFIGS["i_v4_1"]
    n1 = 24001
    kern = {f"edge_nn{nn}": {"launches_per_forward": 8, "avg_launch_ms": ms} for nn, ms in ((8, 0.0626), (16, 0.0937), (32, 0.1554), (64, 0.2705))}
    table, frac_rp = bench.per_nn_table(cfg, kern, n1, None)
    assert sorted(table) == ["16", "32", "64", "8"] and frac_rp == {}
    assert abs(table["64"]["frac_def_A"] - 0.389) < 1e-3 and abs(table["8"]["frac_def_A"] - 0.253) < 1e-3      # the round-3 verdict's table
    assert all(table[k]["frac_def_A_rocprof"] is None and table[k]["traffic"] is None for k in table)
    tf = {"kernels": {"k_edge<64,12,true,4,12>": {"fetch_bytes_per_dispatch_raw": 80.0e6, "write_bytes_per_dispatch": 72.0e6}},
          "rocprof_kernel_trace": {"kernels": {"k_edge<64,12,true,4,12>": {"calls": 136, "avg_ns": 300400.0}}}}
    table, frac_rp = bench.per_nn_table(cfg, kern, n1, tf)
    assert abs(frac_rp[64] - 0.350) < 1e-3 and abs(table["64"]["rocprof_avg_launch_ms"] - 0.3004) < 1e-6
    assert abs(table["64"]["traffic"] - 232.0e6) < 1 and abs(table["64"]["traffic_over_compulsory"] - 232.0e6 / (1280.0 * n1)) < 1e-9
    assert table["8"]["frac_def_A_rocprof"] is None
    # what the fabric actually carried, the clock under the kernel and the issue-floor ratio ride in the same stamped file
    assert abs(table["64"]["hbm_actual_frac"] - 232.0e6 / 0.2705e-3 / 8e12) < 1e-9 and table["64"]["clock_GHz"] is None
    tf["issue_floor"] = {"per_nn": {"64": {"clock_GHz": 2.16, "predicted_us": 241.8, "measured_us": 243.6, "measured_over_predicted": 1.007}}}
    table, _ = bench.per_nn_table(cfg, kern, n1, tf)
    assert table["64"]["clock_GHz"] == 2.16 and abs(table["64"]["issue_floor_ratio"] - 270.5 / 241.8) < 1e-9 and table["8"]["issue_floor_ratio"] is None
    src = open(os.path.join(ROOT, "bench.py")).read()
    for key in ('"hbm_actual_frac"', '"issue_floor_ratio"', '"clock_GHz"', '"frac_of_fp32_mfma_peak"', '"bound_note"', '"segment_call"', '"call": "Model.forward(X, ids_topk, q, M)"',
                '"live_clock"', '"sclk_GHz_mean"', '"mask_pass_ms_per_step"'):
        assert key in src, key
    assert 'else "issue"' in src      # neither pipe half used: the line says instruction issue binds, not hbm
    assert '"frac_rocprof"' in src and '"per_nn"' in src and "speedup_vs_reference_equivalent_cpu_estimate" in src
    assert 'out["speedup_vs_reference_equivalent_cpu"]' not in src


def test_dump_outputs_writes_float32_npy(tmp_path):
    """--dump-outputs: one <name>.npy per array, float32 (float64 kept), from numpy arrays and torch tensors alike."""
    import numpy as np
    import torch
    bench.dump_outputs(str(tmp_path / "d"), {"z": torch.arange(6, dtype=torch.float16).reshape(3, 2), "w": np.ones(4), "v": np.arange(3)})
    z, w, v = (np.load(str(tmp_path / "d" / f"{n}.npy")) for n in ("z", "w", "v"))
    assert z.dtype == np.float32 and z.shape == (3, 2) and z[2, 1] == 5.0
    assert w.dtype == np.float64 and v.dtype == np.float32 and sorted(os.listdir(str(tmp_path / "d"))) == ["v.npy", "w.npy", "z.npy"]
