#!/usr/bin/env python3
"""bench.py - structures/s of the PeSTo forward pass (i_v4_1 architecture) on MI355X.

Contract (driver):  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]   -> ONE JSON line on rank 0.
  * a plain run does only what the headline needs: set-up, clock pre-roll, W warm-up steps, the K timed steps, the outputs of the
    last timed step (--dump-outputs), the line (metric, value, unit, higher_is_better, dtype, ms_per_step = ms of one timed step).
    Every side measurement and check below (roofline, whole_forward, long_sample, segment_call, batch1 latency, exact fp32, the
    config-4 legs, the CPU baseline, the parity check against the reference golden, per-rank times) runs with --full only; without
    it their keys are null;
  * --dump-outputs DIR: after the timed steps, the logits z [sum R, 5] of the last timed step as DIR/z.npy (float32; rank r > 0 of a
    multi-rank run: DIR/z_rank<r>.npy; with --mode strong also the gathered config-4 logits as DIR/config4_z.npy). The inputs are
    seeded: the same arguments give the same inputs in every run;
  * one "step" = one call of the reference's own signature, Model.forward(X, ids_topk, q, M), over one collated batch of --batch
    synthetic structures (N=3000 atoms, k=64, R=375 each; BASELINE.json configs[1]) with every input - the dense fp32 mask M
    included - already resident in HBM (the mask is reduced to residue segments on the GPU inside the call);
  * --gpus N > 1 under plain `python` re-executes itself under torch.distributed.run with N ranks (one per GPU, RCCL);
    under the driver's own torch.distributed.run launch it reads RANK / LOCAL_RANK / WORLD_SIZE. Structures are independent,
    so each rank owns its own batch (weak scaling, no data-path collective); RCCL carries the barrier and the max-over-ranks time;
  * value = structures processed by all ranks / max-over-ranks wall time of the K timed steps.
Extra objects in the same line:
  roofline        the dominant kernel (k_edge<64>), HIP-event timed inside the library on the launch stream: gather-counted
                  algorithmic bytes per launch / duration against 8 TB/s (`frac`, SURVEY 8d definition A), the bytes that actually
                  reached the fabric against the same peak (`hbm_actual_frac`), executed MFMA FLOP/s against the f16 pipe's peak, and
                  what binds (`bound`: "issue" when neither exceeds one half - then `issue_floor_ratio` = launch time / the priced sum
                  of the instructions the launch issues, at the `clock_GHz` the kernel held); the profile-derived keys come from the
                  committed, hash-stamped PMC passes of this build (null when stale);
  cpu_baseline    the C oracle (a port of the reference CPU path) on this host's cores, bounded sample, plus the
                  reference-equivalent time rho x t_port (rho measured in the build container, profiles/r06_cpu_rho.json);
  config4_sharded BASELINE config 4 as a strong-scaling leg: a FIXED list of 64 structures with the pdbs_test size histogram
                  through pesto_amd.sharding.forward_sharded (nccl, device tensors in the gather), gathered z checked bitwise
                  against a world-1 run (--mode strong makes this leg the headline value);
  value_exact_fp32, exact_fp32, parity_max_abs: the same step on the exact fp32 MFMA kernels (with their fraction of the 157.3 TF
                  fp32-MFMA peak per kernel); the timed output against the committed reference golden of structure 0.
"""
import argparse
import hashlib
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# /opt/skills/guides/MI355X_MICROARCH.md
PEAK_F32_TFLOPS = 157.3   # fp32 matrix = vector peak
PEAK_HBM_GBS = 8000.0     # HBM3E spec (6.3 TB/s achievable with a float4 copy; profiles/microbench/r02_peaks.txt has this box's figure)
PEAK_F16_TFLOPS = 2500.0  # dense f16 MFMA: the pipe the split GEMMs run on

# atoms per chain of the reference's pdbs_test/ (53 chains, 1,641-3,052 atoms, sum 132,417): BASELINE config 4's size histogram
# (tests/golden/pdbs_test_sizes.npz holds the same numbers with the chain names)
PDBS_TEST_ATOMS = [1641, 1844, 1869, 1887, 1933, 2046, 2087, 2163, 2196, 2205, 2230, 2246, 2280, 2327, 2351, 2371, 2386, 2412, 2423,
                   2432, 2448, 2448, 2448, 2451, 2467, 2493, 2500, 2500, 2538, 2552, 2591, 2627, 2627, 2629, 2645, 2647, 2647, 2683,
                   2715, 2744, 2775, 2810, 2810, 2810, 2824, 2849, 2878, 2899, 2967, 2970, 2993, 3051, 3052]


def layer_flops_per_atom(nn):
    """Reference-formulation FLOPs per atom per layer: 2*(13,696 + 36,376*n)."""
    return 2.0 * (13696.0 + 36376.0 * nn)


def edge_mfma_flops_per_atom(nn):
    """FLOPs the matrix cores execute per centre atom in the shipped edge kernel. Per 16-edge tile: 8 (16 when nn = 8) fp32 16x16x4
    MFMAs (1,024 MAC: the centre terms) + 90 f16 16x16x32 MFMAs (8,192 MAC; 3 products of the hi/lo split: 24 for the p_j.r block of
    layer 1, 18 key networks, 48 value network). Finish phase inside the kernel: 60 f16 MFMAs per 16 centres (qpm 24, ppm 36)."""
    per_tile = ((16 if nn == 8 else 8) * 1024 + 90 * 8192) * 2.0
    return nn / 16.0 * per_tile + 60 * 8192 * 2.0 / 16.0


# a layer's records ([U|A] 96 + G 72 + nqm 21 f16 MFMAs per 16 atoms): written by the prepare phase of the PREVIOUS layer's edge launch
# (layer 0: by the one k_node16 launch of a forward)
NODE_MFMA_FLOPS_PER_ATOM = 189 * 8192 * 2.0 / 16.0


def executed_mfma_flops(config, n1):
    """per forward: edge kernels (with their finish phase) + one set of records per layer (node kernel / prepare phases)."""
    return sum(edge_mfma_flops_per_atom(l["nn"]) + NODE_MFMA_FLOPS_PER_ATOM for l in config["sum"]) * n1


def exact_edge_mfma_flops_per_atom(nn):
    """FLOPs the matrix cores execute per centre atom in the EXACT fp32 edge kernel (k_edge<..., F16 = false>): per edge, layers 2 / 3 of
    the three edge MLPs (eq 32x32 + ep 32x32 + ev 64x64; keys 64 -> 16 rows, values 64 x 64) and the centre terms (128 features x K = 4,
    twice at nn = 8: two centres share a tile); the neighbour terms of layer 1 are VALU work there (full 2 KB records)."""
    return nn * 2.0 * (6144.0 + 1024.0 + 4096.0 + 512.0 * (2 if nn == 8 else 1))


# k_node (exact): finish (qpm 64-32-32-32, ppm 3 x 64-32) + records ([U|A] 64-256, [G|C] 3 x 32-256, nqm 64-32-32-16) per atom and layer
EXACT_NODE_MFMA_FLOPS_PER_ATOM = 2.0 * (4096.0 + 6144.0 + 16384.0 + 24576.0 + 3584.0)


def layer_gather_bytes_per_atom(nn):
    """Gather-counted bytes per atom per layer (definition A): 1,024 + 532*n."""
    return 1024.0 + 532.0 * nn


def per_nn_table(config, kern, n1, traffic_file):
    """{nn: launch time by HIP events, def-A fraction by events and by the committed rocprofv3 trace, HBM-side traffic per launch,
    traffic / compulsory bytes (def. B)} for every layer kernel of the forward; the profile-derived entries are None unless the
    committed profile carries the source hash of this build."""
    table, frac_rp = {}, {}
    for nn in sorted({l["nn"] for l in config["sum"]}):
        k = kern.get(f"edge_nn{nn}")
        if not k:
            continue
        b_a = layer_gather_bytes_per_atom(nn) * n1
        row = {"avg_launch_ms": k["avg_launch_ms"], "launches_per_forward": k["launches_per_forward"],
               "frac_def_A": b_a / (k["avg_launch_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS,
               "rocprof_avg_launch_ms": None, "frac_def_A_rocprof": None, "traffic": None, "traffic_over_compulsory": None,
               "hbm_actual_frac": None, "clock_GHz": None, "issue_floor_ratio": None}
        if traffic_file:
            hit = [v for kk, v in traffic_file["kernels"].items() if f"k_edge<{nn}," in kk]
            if hit:
                row["traffic"] = 2.0 * hit[0]["fetch_bytes_per_dispatch_raw"] + hit[0]["write_bytes_per_dispatch"]
                row["traffic_over_compulsory"] = row["traffic"] / ((1024.0 + 4.0 * nn) * n1)
                row["hbm_actual_frac"] = row["traffic"] / (k["avg_launch_ms"] * 1e-3) / 1e9 / PEAK_HBM_GBS
            fl = traffic_file.get("issue_floor", {}).get("per_nn", {}).get(str(nn))
            if fl:      # (profiles/issue_floor.py: the clock of the profiled dispatch; the ratio re-taken with THIS run's launch time)
                row["clock_GHz"] = fl["clock_GHz"]
                row["issue_floor_ratio"] = k["avg_launch_ms"] * 1e3 / fl["predicted_us"]
            tr = [v for kk, v in traffic_file.get("rocprof_kernel_trace", {}).get("kernels", {}).items() if f"k_edge<{nn}," in kk]
            if tr:
                row["rocprof_avg_launch_ms"] = tr[0]["avg_ns"] * 1e-6
                row["frac_def_A_rocprof"] = b_a / (tr[0]["avg_ns"] * 1e-9) / 1e9 / PEAK_HBM_GBS
                frac_rp[nn] = row["frac_def_A_rocprof"]
        table[str(nn)] = row
    return table, frac_rp


def make_batch(n_atoms, batch, seed0, n0, order="random"):
    from concurrent.futures import ThreadPoolExecutor
    from pesto_amd.topology import collate_batch_features, mask_to_segments, synthetic_structure
    # the structures are independent and seeded: built on a few threads (the dense host topology's numpy sort releases the GIL), the
    # same arrays as one after the other - set-up time outside the timed steps
    with ThreadPoolExecutor(max_workers=max(1, min(batch, 8))) as ex:
        items = list(ex.map(lambda b: list(synthetic_structure(n_atoms, seed0 + b, n0=n0, order=order)), range(batch)))
    X, ids, q, M = collate_batch_features(items)
    roa, R = mask_to_segments(M)
    return X, ids, q, roa, R


def load_weights(config):
    """i_v4_1 architecture with stacked real i_v4_0 weights (the trained i_v4_1 blob is absent upstream)."""
    from pesto_amd.weights import stack_layers, synthetic_state_dict
    path = os.path.join(ROOT, "tests", "golden", "weights_i_v4_0.npz")
    if len(config["sum"]) == 32 and os.path.exists(path):
        d = np.load(path)
        return stack_layers({k: d[k] for k in d.files}, config, 0.5), "stacked i_v4_0 (real) weights"
    return synthetic_state_dict(config, seed=0), "seeded random weights"


def source_hash():
    """sha256 over the kernel sources: stamps the PMC-derived traffic file so that a stale one is detectable."""
    h = hashlib.sha256()
    for f in ("pesto_node.hip", "pesto_edge.hip", "pesto_mfma_common.h", "pesto_fin_rendezvous.inc", "pesto_edge_node_waves.inc", "pesto_kernels.hip", "pesto_api.hip", "pesto_schema.cpp", "pesto_schema.h", "pesto_kernels.h"):
        h.update(open(os.path.join(ROOT, "pesto_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:16]


def cpu_quota_cores():
    """CPUs the cgroup lets this process USE at once (cpu.max quota / period; cgroup v1: cfs_quota_us / cfs_period_us), or None when
    unlimited / unknown. A box that shows 256 CPUs under a quota of 32 runs 256 OpenMP threads on 32 cores' worth of time."""
    for q_path, p_path in (("/sys/fs/cgroup/cpu.max", None), ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us")):
        try:
            if p_path is None:
                q_, p_ = open(q_path).read().split()[:2]
            else:
                q_, p_ = open(q_path).read().strip(), open(p_path).read().strip()
            if q_ != "max" and float(q_) > 0:
                return float(q_) / float(p_)
        except (OSError, ValueError):
            continue
    return None


def oracle_source_sha16():
    return hashlib.sha256(open(os.path.join(ROOT, "oracle", "pesto_oracle.c"), "rb").read()).hexdigest()[:16]


def cpu_baseline(config, sd, n_atoms, budget_s, config_key):
    """The C oracle (port of the reference CPU path, OpenMP over atoms) on this host's cores, bounded sample: once on ALL cores
    (the headline `value`) and once on the thread count rho was measured at (8), so that the reference-equivalent time
    rho x t_port multiplies a time taken at EQUAL threads (the two do not commute: the port scales sub-linearly)."""
    from oracle import oracle
    X, ids, q, roa, R = make_batch(n_atoms, 1, 1, config["em"]["N0"])
    m = oracle.OracleModel(config, sd)
    ids32 = ids.astype(np.int32)
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    omp = os.environ.get("OMP_NUM_THREADS")
    all_threads = int(omp) if omp else cores

    def sample(threads, budget, max_n):
        oracle.set_threads(threads)
        t0 = time.perf_counter()
        m.forward_segments(X, ids32, q, roa, R, stop_after=2)     # touch pages / spin up the OpenMP team
        t_warm = time.perf_counter() - t0
        times = []
        t_start = time.perf_counter()
        while not times or (time.perf_counter() - t_start + np.mean(times) < budget and len(times) < max_n):
            t0 = time.perf_counter()
            m.forward_segments(X, ids32, q, roa, R)
            times.append(time.perf_counter() - t0)
        return float(np.median(times)), len(times), t_warm

    # the port is timed at doubling team sizes up to the CPUs the process may use; the headline is its BEST team size. Where the curve
    # stops falling is stated with its reason: the cgroup's CPU quota (a box can show 256 CPUs and grant 32 cores' worth of time) or,
    # without a quota, the port itself (3,001 equal atoms per layer, one OpenMP loop: memory-bound gathers beyond ~32 threads)
    quota = cpu_quota_cores()
    sizes_ = sorted({v for v in (8, 16, 32, 64, 128, 256) if v < all_threads} | {all_threads})
    tried = {}
    for thr_ in sizes_:
        tried[thr_] = sample(thr_, 0.4 * budget_s / len(sizes_), 3)
        if tried[thr_][0] > 3.0 * min(v_[0] for v_ in tried.values()):      # far beyond the knee: larger teams only cost sample time
            break
    best = min(tried, key=lambda k_: tried[k_][0])
    t, n, t_warm = tried[best]
    why = (f"cgroup CPU quota = {quota:.0f} cores' worth of time on a host that shows {cores} CPUs" if quota and quota < 0.9 * cores else
           f"no CPU quota: the port itself stops scaling there (one OpenMP loop over {n_atoms + 1} atoms per layer, gather-bound)")
    out = {"value": 1.0 / t, "unit": "structures/s", "cores": best, "kind": "port",
           "sample": f"{n} x one N={n_atoms} structure, all {len(config['sum'])} layers, C oracle (OpenMP, passive waits, {best} threads = the best of "
                     f"{sorted(tried)} on this host's {cores} CPUs; {why}); median {t:.2f} s/structure (2-layer warm-up {t_warm:.2f} s)",
           "cores_why": why, "cpu_quota_cores": quota, "host_cpus": cores,
           "seconds_per_structure_by_threads": {str(k_): v_[0] for k_, v_ in sorted(tried.items())}}
    # reference-equivalent CPU time = rho x t_port, rho = t_reference / t_port measured on equal cores in the
    # build container (profiles/cpu_rho.py -> profiles/r06_cpu_rho.json, copied to BASELINE.md) and applied to the port's time at
    # THAT thread count on this host
    rpath = os.path.join(ROOT, "profiles", "r06_cpu_rho.json")
    if os.path.exists(rpath):
        r = json.load(open(rpath))
        hit = [v for k, v in r["configs"].items() if k.startswith(config_key)]
        if r.get("oracle_source_sha16") != oracle_source_sha16():
            # rho = reference / port on equal cores is a property of THIS port: a ratio measured with another oracle source is refused
            out["reference_equivalent"] = None
            out["reference_equivalent_note"] = (f"profiles/r06_cpu_rho.json was measured with oracle source {r.get('oracle_source_sha16')}, the oracle "
                                                f"timed here is {oracle_source_sha16()}: re-run profiles/cpu_rho.py in the build container")
        elif hit:
            rho = float(np.mean([v["rho"] for v in hit]))
            thr = int(r["threads"])
            t8, n8, _ = sample(min(thr, all_threads), 0.4 * budget_s, 3)
            oracle.set_threads(all_threads)
            out["port_at_rho_threads"] = {"threads": min(thr, all_threads), "seconds_per_structure": t8, "structures_per_s": 1.0 / t8,
                                          "sample": f"{n8} x the same structure", "speedup_of_the_best_team_over_these": t8 / t}
            out["reference_equivalent"] = {"rho": rho, "threads": min(thr, all_threads), "seconds_per_structure": rho * t8,
                                           "structures_per_s": 1.0 / (rho * t8),
                                           "estimate": True, "rho_machine": "build container (no GPU), not this host",
                                           "provenance": f"rho = reference PyTorch CPU time / C-oracle time on the same {thr} threads of the "
                                                         f"build container (torch {r['torch']}), profiles/r06_cpu_rho.json (oracle source {r['oracle_source_sha16']}), times the port's "
                                                         f"time at {min(thr, all_threads)} threads on THIS host; the reference itself cannot "
                                                         "run on the GPU box"}
    return out


def config4_structures(n_structures, model=None, forms="compact"):
    """The work list of BASELINE config 4: the chains of the reference's pdbs_test/ (53 chains, 1,641 - 3,052 atoms; coordinates,
    features, residue maps and the reference's logits are the parity fixture tests/golden/cfg4_all53.npz), repeated cyclically when
    more structures are asked for. Without the fixture: synthetic structures with the same size histogram.
    With a model the neighbour tables come from the GPU k-NN (pesto_knn_collate: the same exact table as the host contract, tested
    entry for entry on these chains; 64 structures in milliseconds instead of ~0.5 s of dense host work each).
    forms: "compact" = what a loader that keeps encode_features' argmax hands over (uint8 feature indices, res_of_atom, uint16 ids -
    reduced HERE, outside every timed region); "dense" = the reference loader's own outputs per structure, untouched: float32 one-hot q
    (encode_features, src/data_encoding.py:78-84), BOOL mask M (encode_structure, :61-75), int64 ids (extract_topology, :87-102) - every
    reduction (one-hot detection, mask -> segments, id narrowing) then happens inside the timed submit.
    Returns (structures, sizes, reference logits per structure or None)."""
    from pesto_amd.topology import synthetic_structure
    fx = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tests", "golden", "cfg4_all53.npz")
    refs = None
    if os.path.exists(fx) and model is not None and model.config["em"]["N0"] == 30:
        g = np.load(fx)
        ao, ro = g["atom_offsets"], g["res_offsets"]
        n_chains = len(g["names"])
        items, sizes, refs = [], [], []
        for i in range(n_structures):
            c = i % n_chains
            X = np.ascontiguousarray(g["X"][ao[c]:ao[c + 1]])
            n = X.shape[0]
            q = np.zeros((n, 30), np.float32)
            q[np.arange(n), g["q_idx"][ao[c]:ao[c + 1], 0]] = 1.0
            roa = g["res_of_atom"][ao[c]:ao[c + 1]].astype(np.int64)
            M = np.zeros((n, int(ro[c + 1] - ro[c])), np.float32)
            M[np.arange(n), roa] = 1.0
            items.append([X, None, q, M]); sizes.append(n); refs.append(g["z"][ro[c]:ro[c + 1]])
        if len(model.config["sum"]) != 32:      # the fixture's logits are the i_v4_1 architecture's (stacked weights, load_weights)
            refs = None
    else:
        sizes = [PDBS_TEST_ATOMS[i % len(PDBS_TEST_ATOMS)] for i in range(n_structures)]
        items = [list(synthetic_structure(n, 5000 + i, topology=model is None)) for i, n in enumerate(sizes)]
    if model is not None:
        ids = model.knn_collate(np.concatenate([it[0] for it in items]), sizes)          # [sum N, 64], 1-based batch-global
        off = 0
        for it, n in zip(items, sizes):
            it[1] = (ids[off:off + n] - (off + 1)).astype(np.int32)                      # 0-based within the structure (N >= 64: no padding)
            off += n
        if refs is not None:
            # 21 rows of these chains hold two neighbours at exactly the same fp32 distance; torch.topk put them the other way round
            # than the index order of the k-NN (one pair straddles the nn = 32 cut-off): take the reference's choice there, so that the
            # parity check below compares like with like (fixture's patch list: chain, row, slot, 0-based id)
            for c, r, col, v in g["tie_patches"]:
                for i in range(int(c), n_structures, n_chains):
                    items[i][1][r, col] = v
    if forms == "dense":
        for it in items:
            it[1] = np.ascontiguousarray(it[1].astype(np.int64)) if it[1] is not None else None
            it[3] = np.ascontiguousarray(it[3] > 0.5)
    elif model is not None and model.config["em"]["N0"] == 30:
        # the compact per-structure forms of forward_batch_submit, as a loader would hand them over (encode_features' argmax, the residue
        # column per atom, uint16 neighbour ids): the Python layer then touches no array element and the library packs bytes
        for it in items:
            it[1] = it[1].astype(np.uint16) if it[0].shape[0] <= 65536 else it[1]
            it[2] = np.ascontiguousarray(it[2].argmax(1).astype(np.uint8)[:, None])
            it[3] = np.ascontiguousarray(it[3].argmax(1).astype(np.int32))
    return [tuple(it) for it in items], sizes, refs


def config4_leg(model, dist, backend, dev, n_structures, reps, max_atoms, forms="compact", fixed_list=False, outputs=None):
    """The config-4 work list sharded by pesto_amd.sharding (LPT partition, per-rank launches of <= max_atoms atoms from host memory,
    ragged all_gather of the logits). fixed_list=False: n_structures grows with the world size (weak); True: the SAME list at every world
    size (SURVEY 8e's acceptance: >= 7x on 8 GPUs for a list of >= 64 structures), with a world-1 pass of the list on rank 0 timed beside
    it (`speedup_vs_world1`). Returns the leg's result dict on rank 0; with a dict `outputs`, rank 0 also puts the gathered logits of the
    last timed pass there (key "config4_z": the structures' logits concatenated in list order)."""
    import torch
    from pesto_amd import sharding
    structures, sizes, refs = config4_structures(n_structures, model, forms)
    n_out = model.config["dm"]["N2"]
    rank = dist.get_rank() if dist is not None else 0
    world = dist.get_world_size() if dist is not None else 1

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    gathered = sharding.forward_sharded(model, structures, n_out, max_atoms=max_atoms)       # warm-up (workspace growth, RCCL setup)
    times, per_rank = [], []
    for _ in range(reps):
        barrier()
        t0 = time.perf_counter()
        c0 = time.process_time()
        tm = {}
        gathered = sharding.forward_sharded(model, structures, n_out, max_atoms=max_atoms, timings=tm)
        cpu_s = time.process_time() - c0
        barrier()
        el = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        times.append(el)
        per_rank.append(gather_rank_stats(dist, backend, dev, [tm["local_s"], tm["gather_s"], cpu_s, tm["structures"], tm["atoms"]]))
    # world-1 pass of the same list on rank 0 alone (the other ranks wait at the barrier): the denominator of the fixed-list speed-up
    t_world1 = None
    if fixed_list:
        barrier()
        if rank == 0:
            sharding.forward_local(model, structures, list(range(len(structures))), max_atoms=max_atoms)
            torch.cuda.synchronize()
            t1s = []
            for _ in range(max(2, reps // 2)):
                t0 = time.perf_counter()
                sharding.forward_local(model, structures, list(range(len(structures))), max_atoms=max_atoms)
                torch.cuda.synchronize()
                t1s.append(time.perf_counter() - t0)
            t_world1 = float(np.median(t1s))
        barrier()
    if rank != 0:
        return None
    if outputs is not None:
        outputs["config4_z"] = np.concatenate([np.asarray(g, dtype=np.float32) for g in gathered])
    # world-1 run of the same list on this rank; every structure must come back with the same bits (PESTO_BATCH_INDEPENDENT)
    local = sharding.forward_local(model, structures, list(range(len(structures))), max_atoms=max_atoms)
    ok = all(g is not None and np.array_equal(g, local[i]) for i, g in enumerate(gathered))
    t_med = float(np.median(times))
    # the timed output against the REFERENCE's logits of the same chains (neighbour tables from the GPU k-NN: they differ from the
    # reference's in the order of exact distance ties only)
    parity = None if refs is None else float(max(np.abs(g - r).max() for g, r in zip(gathered, refs)))
    assert parity is None or parity < 1e-4, parity
    what = (f"{len(structures)} real chains of the reference's pdbs_test/ set (53 distinct, repeated cyclically; " if refs is not None
            else f"{len(structures)} synthetic structures with the pdbs_test size histogram (")
    return {"workload": what + f"{min(sizes)}-{max(sizes)} atoms, "
                        f"{sum(sizes)} atoms in total), i_v4_1, list sharded over {world} rank(s) by atom count (LPT), launches of <= "
                        f"{max_atoms} atoms, inputs in HOST memory (packing + H2D inside the timed region, two launches in flight: "
                        f"pesto_forward_batch_submit / _wait), logits all-gathered to every rank "
                        f"({backend if world > 1 else 'no collective at world 1'})",
            "inputs": ("dense: the reference loader's per-structure outputs as they are - float32 one-hot q, bool mask M, int64 ids; one-hot detection, "
                       "mask -> segments and id narrowing INSIDE the timed region" if forms == "dense" else
                       "compact, pre-reduced OUTSIDE the timed region: uint8 feature indices (argmax of q), res_of_atom (the member column of M), uint16 ids"),
            "structures": len(structures), "structures_per_rank": len(structures) // world, "value": len(structures) / t_med, "unit": "structures/s",
            "scaling": ("strong (the same list at every world size)" if fixed_list else
                        "weak (the list grows with the world size: a fixed number of structures per rank)"),
            "seconds_world1_on_rank0": t_world1, "speedup_vs_world1": None if t_world1 is None else t_world1 / t_med,
            "seconds_per_pass_median": t_med, "passes": reps, "bitwise_equal_to_world1": bool(ok), "parity_max_abs_vs_reference": parity,
            # per rank (median over the passes): seconds in its own launches, seconds waiting in / doing the result gather, CPU seconds of
            # the rank's process (packing, submit / wait, gather), its share of the list - a straggler or a starved host shows here
            "per_rank": [{"rank": r, "local_s": float(np.median([p[r][0] for p in per_rank])), "gather_s": float(np.median([p[r][1] for p in per_rank])),
                          "host_cpu_s": float(np.median([p[r][2] for p in per_rank])), "structures": int(per_rank[0][r][3]), "atoms": int(per_rank[0][r][4]),
                          "structures_per_s": float(per_rank[0][r][3] / np.median([p[r][0] for p in per_rank]))} for r in range(world)],
            "rank_local_s_max_over_min": float(max(np.median([p[r][0] for p in per_rank]) for r in range(world)) /
                                               max(1e-12, min(np.median([p[r][0] for p in per_rank]) for r in range(world)))),
            "host_cpu_s_per_structure": float(np.median([sum(p[r][2] for r in range(world)) for p in per_rank]) / len(structures))}


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array (torch tensor or numpy) as <out_dir>/<name>.npy in float32 (float64 stays float64)."""
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        a = a.detach().cpu().numpy() if hasattr(a, "detach") else np.asarray(a)
        np.save(os.path.join(out_dir, name + ".npy"), a if a.dtype == np.float64 else a.astype(np.float32))


def gather_rank_stats(dist, backend, dev, values):
    """[values of rank 0, values of rank 1, ...] on every rank (a list of floats per rank; no process group: just this process)."""
    import torch
    if dist is None:
        return [list(map(float, values))]
    t = torch.tensor(values, dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
    out = [torch.empty_like(t) for _ in range(dist.get_world_size())]
    dist.all_gather(out, t)
    return [[float(v) for v in o.cpu()] for o in out]


def self_launch(args):
    """`python bench.py --gpus N` without a launcher: become N ranks under torch.distributed.run (one per GPU)."""
    import torch
    if not args.same_gpu and torch.cuda.device_count() < args.gpus:
        msg = (f"bench.py --gpus {args.gpus}: only {torch.cuda.device_count()} GPU(s) visible "
               "(--same-gpu with --backend gloo runs the multi-rank path on one GPU, for testing)")
        print(json.dumps({"metric": "structures/sec (N=3000 atoms, k=64, 32 layers)", "value": None, "unit": "structures/s", "n_gpus": args.gpus,
                          "steps": args.steps, "warmup": args.warmup, "error": msg, "error_stage": "self launch", "visible_gpus": int(torch.cuda.device_count())}), flush=True)
        raise SystemExit(msg)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    raise SystemExit(subprocess.call(cmd, env=env))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--preroll-ms", type=float, default=100.0,
                    help="untimed run of the same step IN FRONT of the warm-up steps until this much time has passed: an idle MI355X takes "
                         "~30 ms of work to reach its steady clocks (profiles/r05_clock_ramp.txt); the host-side set-up leaves it idle. 0 = none")
    ap.add_argument("--batch", type=int, default=8, help="structures per step per GPU")
    ap.add_argument("--atoms", type=int, default=3000)
    ap.add_argument("--config", default="i_v4_1")
    ap.add_argument("--mode", default="weak", choices=["weak", "strong"],
                    help="headline value: weak = config 2 replicated per rank; strong = the config-4 work list sharded over the ranks")
    ap.add_argument("--precision", default="auto", choices=["auto", "f16_split", "fp32"], help="pesto_precision of the timed steps")
    ap.add_argument("--full", action="store_true",
                    help="also run every side measurement and check (roofline, whole forward, 200-step sample, segment call, batch-1 "
                         "latency, exact fp32, config-4 legs, CPU baseline, parity against the reference golden); a plain run times "
                         "the headline steps only")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the logits of the last timed step as DIR/z.npy (float32) after the timed steps")
    ap.add_argument("--cpu-budget", type=float, default=20.0, help="--full: seconds of CPU-baseline work (0 = skip)")
    ap.add_argument("--no-latency", action="store_true", help="--full: skip the batch-1 latency side measurement")
    ap.add_argument("--no-check", action="store_true", help="developer ablation builds only: do not check the timed output")
    ap.add_argument("--no-extras", action="store_true", help="--full: skip the exact-fp32 and config-4 legs (profiling runs)")
    ap.add_argument("--config4-structures", type=int, default=64, help="structures PER RANK of the config-4 leg (the list has this many x world size)")
    ap.add_argument("--config4-max-atoms", type=int, default=24576, help="atoms per collated launch of the config-4 legs (sharding.forward_sharded)")
    ap.add_argument("--strong-structures", type=int, default=512, help="size of the FIXED list of the config4_strong leg (N > 1 only)")
    ap.add_argument("--backend", default="nccl", choices=["nccl", "gloo"], help="torch.distributed backend (nccl = RCCL)")
    ap.add_argument("--same-gpu", action="store_true",
                    help="testing only: every rank uses GPU 0 (lets the N>1 code path run on a 1-GPU box with --backend gloo)")
    ap.add_argument("--no-numa-bind", action="store_true", help="do not pin the rank to the CPUs of its GPU's NUMA node")
    ap.add_argument("--edge-mode", type=int, default=0, help="developer: pesto_debug_edge_mode (0 = per launch, 1 rendezvous, 2 node waves)")
    ap.add_argument("--order", default="random", choices=["random", "morton"],
                    help="atom numbering of the synthetic clouds: generation order, or along a Z-order curve")
    args = ap.parse_args()
    # the CPU-baseline leg times an OpenMP port at team sizes up to the host's CPU count: under a cgroup CPU quota (or shared vCPUs) an
    # ACTIVE-waiting team of 256 spins its own time slices away (8 s per structure against 0.6 s at 32 threads in round 5). Passive waits,
    # set before any OpenMP runtime is loaded, make the curve flat instead of catastrophic beyond the knee.
    os.environ.setdefault("OMP_WAIT_POLICY", "PASSIVE")
    os.environ.setdefault("GOMP_SPINCOUNT", "2000")

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        self_launch(args)
    stage = ["start"]
    try:
        run(args, stage)
    except SystemExit:
        raise
    except BaseException as e:      # noqa: BLE001 - the driver reads ONE JSON line from stdout: a failure becomes that line, the traceback goes to stderr
        import traceback
        traceback.print_exc(file=sys.stderr)
        if int(os.environ.get("RANK", "0")) == 0:
            print(json.dumps({"metric": "structures/sec (N=3000 atoms, k=64, 32 layers)", "value": None, "unit": "structures/s", "n_gpus": args.gpus,
                              "steps": args.steps, "warmup": args.warmup, "error": f"{type(e).__name__}: {e}"[:600], "error_stage": stage[0],
                              "world_size_env": os.environ.get("WORLD_SIZE"), "local_rank_env": os.environ.get("LOCAL_RANK"),
                              "visible_gpus": _visible_gpus()}), flush=True)
        sys.exit(1)


def _visible_gpus():
    try:
        import torch
        return int(torch.cuda.device_count())
    except Exception:      # noqa: BLE001
        return None


def run(args, stage):

    import torch
    from pesto_amd import Model
    from pesto_amd.config import CONFIGS

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    stage[0] = "device check"
    if args.gpus != world:
        raise RuntimeError(f"--gpus {args.gpus} != WORLD_SIZE {world}")
    if not torch.cuda.is_available():
        raise RuntimeError("bench.py needs an MI355X (no CPU fallback exists for the forward pass)")
    if not args.same_gpu and torch.cuda.device_count() <= local_rank:
        raise RuntimeError(f"rank {rank}: LOCAL_RANK {local_rank} but only {torch.cuda.device_count()} GPU(s) visible")
    gpu = 0 if args.same_gpu else local_rank
    torch.cuda.set_device(gpu)
    dev = torch.device("cuda", gpu)
    # one rank per GPU: pin the rank to the CPUs of its GPU's NUMA node (host packing + H2D of the config-4 legs; no-op where sysfs
    # gives no node - reported per rank in ranks.devices)
    from pesto_amd import sharding as _shn
    numa_info = _shn.bind_rank_to_numa(dev) if not args.no_numa_bind else {"numa_node": None, "cpus_allowed": None, "cpu_list_head": None, "bound": False, "why": "--no-numa-bind"}
    dist = None
    stage[0] = "process group init (torch.distributed, backend %s)" % args.backend
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (the collective libraries announce themselves on stdout - "[Gloo] Rank 0 is connected to ..." - which must carry only the
        # JSON line: file descriptor 1 points at stderr while the process group comes up)
        sys.stdout.flush()
        saved_fd = os.dup(1)
        os.dup2(2, 1)
        try:
            if args.backend == "nccl":
                dist.init_process_group("nccl", device_id=dev)
            else:
                dist.init_process_group("gloo")
            dist.barrier()
        finally:
            sys.stdout.flush()
            os.dup2(saved_fd, 1)
            os.close(saved_fd)

    stage[0] = "weight broadcast / handle creation"
    config = CONFIGS[args.config]
    n0 = config["em"]["N0"]
    # the weights: rank 0 reads them, every rank builds its handle from the BROADCAST blob (one collective over device tensors under RCCL;
    # sharding.broadcast_weights compares a checksum across the ranks) - SURVEY 8e "init: ncclBroadcast(weights)"
    from pesto_amd import sharding as _sh
    sd, wdesc = load_weights(config) if (rank == 0 or world == 1) else (None, None)
    model = Model(config, validate=False, precision=args.precision).to(dev)
    wb = _sh.broadcast_weights(model, sd if rank == 0 else None, src=0, device=dev)
    if wdesc is None:
        wdesc = "weights received from rank 0"
    ranks_info = _sh.describe_ranks(dev, numa=numa_info)
    if args.edge_mode:
        model.debug_edge_mode(args.edge_mode)

    # ---- inputs: one batch per rank, resident in HBM before the timed region
    stage[0] = "timed steps"
    X, ids, q, roa, R = make_batch(args.atoms, args.batch, 1000 * rank + 1, n0, args.order)
    Xd = torch.from_numpy(X).to(dev)
    idsd = torch.from_numpy(ids).to(dev)            # int64, as the reference passes it
    qd = torch.from_numpy(q).to(dev)
    road = torch.from_numpy(roa).to(dev)
    n_atoms_total = X.shape[0]
    # the dense residue mask of the reference's call (collate_batch_features: block-diagonal float [sum N, sum R], src/dataset.py:101,110),
    # resident in HBM like the other inputs (callers pass M.float().to(device), apply_model.ipynb:155)
    Md = torch.zeros((n_atoms_total, R), dtype=torch.float32, device=dev)
    Md[torch.arange(n_atoms_total, device=dev), road.long()] = 1.0

    def step():      # the reference's own signature (model/model.py:32): the mask is reduced to segments on the GPU inside the call
        return model(Xd, idsd, qd, Md)

    def step_segments():      # the same forward with the mask pre-reduced by the caller (an extra key of the line)
        return model.forward_segments(Xd, idsd, qd, road, R)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(n_warm, n_steps):
        z_ = None
        for _ in range(n_warm):
            z_ = step()
        barrier()
        t0_ = time.perf_counter()
        for _ in range(n_steps):
            z_ = step()
        barrier()
        el = time.perf_counter() - t0_
        if dist is not None:
            t = torch.tensor([el], dtype=torch.float64, device=dev if args.backend == "nccl" else "cpu")
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el = float(t.item())
        return el, z_

    def timed_per_rank(n_steps):
        """every rank's OWN time for n_steps (device-synchronised before and after, no barrier in between the ranks' loops)"""
        barrier()
        t0_ = time.perf_counter()
        for _ in range(n_steps):
            step()
        torch.cuda.synchronize()
        own = time.perf_counter() - t0_
        return [r_[0] for r_ in gather_rank_stats(dist, args.backend, dev, [own])]

    # clock pre-roll (disclosed in the line as "preroll"): the set-up above is host work, the GPU is idle and at its idle clocks when the
    # warm-up starts; the first ~30 ms of work after an idle period run 3 - 12 % slower than the steady state (profiles/r05_clock_ramp.txt)
    preroll_steps = 0
    if args.preroll_ms > 0:
        t_pre = time.perf_counter()
        while (time.perf_counter() - t_pre) * 1e3 < args.preroll_ms:
            step()
            torch.cuda.synchronize()
            preroll_steps += 1
    elapsed, z = timed(args.warmup, args.steps)
    if args.dump_outputs:
        dump_outputs(args.dump_outputs, {"z" if rank == 0 else f"z_rank{rank}": z})
    rank_times = timed_per_rank(args.steps) if world > 1 and args.full else None
    assert args.no_check or torch.isfinite(z).all()
    status = model.status()

    # everything below up to the result line is a side measurement or check: --full only (a plain run times the headline steps)
    parity = exact = roofline = whole = long_sample = seg_call = lat_ms = lat_detail = None
    if args.full:
        # ---- the timed output against the reference: structure 0 of rank 0 is the committed golden (seed 1, N=3000, i_v4_1 stacked)
        gpath = os.path.join(ROOT, "tests", "golden", "fwd_i_v4_1_stacked_synth3000.npz")
        if rank == 0 and args.config == "i_v4_1" and args.atoms == 3000 and args.order == "random" and os.path.exists(gpath) and not args.no_check:
            zg = np.load(gpath)["z"]
            parity = float(np.abs(z[:zg.shape[0]].cpu().numpy() - zg).max())
            assert parity < 1e-4, f"timed output differs from the reference golden by {parity}"

        # ---- the same step on the exact fp32 MFMA kernels (what "auto" falls back to)
        if not args.no_extras and args.precision != "fp32":
            model.set_precision("fp32")
            el32, z32 = timed(2, max(3, min(args.steps, 10)))
            model.set_precision(args.precision)
            exact = {"value": max(3, min(args.steps, 10)) * args.batch * world / el32,
                     "max_abs_vs_timed_output": float((z32 - z).abs().max().item())}
            # per-kernel launch times of the exact path (HIP events between consecutive launches) against the fp32 MFMA peak
            model.set_precision("fp32")
            model.set_timing(True, per_kernel=True)
            pk32 = []
            for _ in range(3):
                step_segments()
                torch.cuda.synchronize()
                pk32.append(model.get_kernel_timing())
            model.set_timing(False)
            model.set_precision(args.precision)
            n1_ = X.shape[0] + 1
            ex_k = {}
            for name in pk32[0]:
                n_l = pk32[0][name][1]
                if not n_l:
                    continue
                ms_ = float(np.median([pk[name][0] for pk in pk32])) / n_l
                fl_ = EXACT_NODE_MFMA_FLOPS_PER_ATOM * n1_ * (len(config["sum"]) / n_l) if name == "node" else exact_edge_mfma_flops_per_atom(int(name[7:])) * n1_
                ex_k[name] = {"launches_per_forward": n_l, "avg_launch_ms": ms_, "executed_mfma_TFLOPs": fl_ / (ms_ * 1e-3) / 1e12,
                              "frac_of_fp32_mfma_peak": fl_ / (ms_ * 1e-3) / 1e12 / PEAK_F32_TFLOPS}
            fl_all = sum(exact_edge_mfma_flops_per_atom(l["nn"]) + EXACT_NODE_MFMA_FLOPS_PER_ATOM for l in config["sum"]) * n1_
            t_all32 = sum(v["avg_launch_ms"] * v["launches_per_forward"] for v in ex_k.values()) * 1e-3
            exact["kernels"] = ex_k
            exact["frac_of_fp32_mfma_peak"] = fl_all / t_all32 / 1e12 / PEAK_F32_TFLOPS if t_all32 > 0 else None
            exact["peak_TFLOPs"] = PEAK_F32_TFLOPS
            exact["definition"] = ("FLOPs the matrix cores execute in k_edge<..., F16 = false> (layers 2 / 3 of the edge MLPs and the centre terms; the "
                                   "neighbour terms of layer 1 are VALU work there) and k_node, / time by HIP events / the 157.3 TF fp32 MFMA peak")

        # ---- roofline leg: HIP events around the state-update launches, on the stream they run on
        # (each sample = the LAST of three back-to-back steps: its events are recorded into a busy stream, as in the timed region of the headline;
        #  a step that starts on a drained GPU reads ~1 % longer)
        model.set_timing(True)
        lay_ms = []
        for _ in range(max(5, min(args.steps, 20))):
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            lay_ms.append(model.get_timing())
        # per-kernel pass (one event between consecutive layer launches): average launch duration of every kernel class
        model.set_timing(True, per_kernel=True)
        per_kernel = []
        for _ in range(5):
            for _ in range(3):
                step()
            torch.cuda.synchronize()
            per_kernel.append(model.get_kernel_timing())
        model.set_timing(False)
        kern = {}
        for name in per_kernel[0]:
            n_l = per_kernel[0][name][1]
            if n_l:
                kern[name] = {"launches_per_forward": n_l, "avg_launch_ms": float(np.median([pk[name][0] for pk in per_kernel])) / n_l}
        layers_ms = float(np.median([t["layers_ms"] for t in lay_ms]))
        fwd_all = np.array([t["total_ms"] for t in lay_ms])
        fwd_ms = float(np.median(fwd_all))
        n_launch = lay_ms[0]["n_layer_launches"]
        n1 = n_atoms_total + 1
        flops = sum(layer_flops_per_atom(l["nn"]) for l in config["sum"]) * n1
        gbytes = sum(layer_gather_bytes_per_atom(l["nn"]) for l in config["sum"]) * n1
        # HBM-side bytes from the committed PMC passes of THIS build (profiles/pmc_collect.sh stamps the file with the source hash)
        traffic_file, traffic_note = None, "no PMC file for this workload"
        tpath = os.path.join(ROOT, "profiles", f"traffic_{args.config}_n{args.atoms}_b{args.batch}.json")
        if os.path.exists(tpath) and args.order == "random":
            tf = json.load(open(tpath))
            if tf.get("source_hash") == source_hash():
                traffic_file, traffic_note = tf, f"rocprofv3 --pmc FETCH_SIZE x2 + WRITE_SIZE per dispatch, {os.path.basename(tpath)} (source hash matches this build)"
            else:
                traffic_note = f"{os.path.basename(tpath)} was collected on other kernel sources (hash {tf.get('source_hash')} != {source_hash()}): not quoted"
        # the dominant kernel: k_edge<nn = max>; SURVEY 8d per atom-layer: FLOP 2*(13,696 + 36,376 n), bytes (A) 1,024 + 532 n
        nn_max = max(l["nn"] for l in config["sum"])
        dom = kern.get(f"edge_nn{nn_max}")
        if dom:
            t_s = dom["avg_launch_ms"] * 1e-3
            b_a = layer_gather_bytes_per_atom(nn_max) * n1
            # launches of this kernel that also write the next layer's records (every layer but the last has a successor)
            n_dom = sum(1 for l in config["sum"] if l["nn"] == nn_max)
            n_prep = sum(1 for i, l in enumerate(config["sum"]) if l["nn"] == nn_max and i + 1 < len(config["sum"]))
            f_exec = n1 * (edge_mfma_flops_per_atom(nn_max) + NODE_MFMA_FLOPS_PER_ATOM * n_prep / n_dom)
            f_ref = 2.0 * 36376.0 * nn_max * n1
            hbm_frac = b_a / t_s / 1e9 / PEAK_HBM_GBS
            mfma_frac = f_exec / t_s / 1e12 / PEAK_F16_TFLOPS
            t_all = sum(v["avg_launch_ms"] * v["launches_per_forward"] for v in kern.values())
            traffic = None
            if traffic_file:
                hit = [v for k, v in traffic_file["kernels"].items() if f"k_edge<{nn_max}," in k]
                if hit:
                    traffic = 2.0 * hit[0]["fetch_bytes_per_dispatch_raw"] + hit[0]["write_bytes_per_dispatch"]
            per_nn, frac_rocprof = per_nn_table(config, kern, n1, traffic_file)
            dom_row = per_nn.get(str(nn_max), {})
            hbm_actual = dom_row.get("hbm_actual_frac")
            # what binds: the matrix pipe or the fabric only when one of them is at least half used. The achieved / peak / frac keys keep SURVEY
            # 8d's definition (A) - gather-counted bytes against the HBM peak, a cache-bandwidth figure - whatever `bound` says; with neither
            # pipe half used the kernel is bound by the NUMBER of instructions it issues (issue_floor_ratio prices them)
            bound = "mfma" if mfma_frac >= 0.5 else ("hbm" if (hbm_actual if hbm_actual is not None else hbm_frac) >= 0.5 else "issue")
            roofline = {
                "kernel": f"k_edge<{nn_max}> = one whole state-update layer: edges, attention, the layer's output MLPs (finish phase) and the next "
                          f"layer's per-atom records (prepare phase) (dominant: {dom['avg_launch_ms'] * dom['launches_per_forward'] / t_all:.0%} of the layer time)",
                "bound": bound,
                "bound_note": "issue = instruction issue: the fabric sees hbm_actual_frac of its peak, the matrix cores run at mfma.frac of theirs; "
                              "achieved / peak / frac are SURVEY 8d's definition (A) (algorithmic gather-counted bytes / launch time / 8 TB/s)",
                "achieved": f_exec / t_s / 1e12 if bound == "mfma" else b_a / t_s / 1e9,
                "peak": PEAK_F16_TFLOPS if bound == "mfma" else PEAK_HBM_GBS,
                "unit": "TFLOP/s" if bound == "mfma" else "GB/s",
                "frac": mfma_frac if bound == "mfma" else hbm_frac,
                # traffic / launch time / 8 TB/s: what the fabric actually carried (committed PMC passes of this build)
                "hbm_actual_frac": hbm_actual,
                # launch time / (dynamic instruction classes of the launch x the micro-benchmark price list at the clock of the profiled dispatch)
                "issue_floor_ratio": dom_row.get("issue_floor_ratio"),
                "clock_GHz": dom_row.get("clock_GHz"),
                # the same fraction from the COMMITTED rocprofv3 kernel trace (average duration of this kernel in the hash-stamped profile
                # of this build, profiles/traffic_*.json; the profiler adds ~5 % to a launch and the trace may come from another box of
                # the pool): null when the committed profile was taken on other kernel sources
                "frac_rocprof": frac_rocprof.get(nn_max) if bound != "mfma" else None,
                "traffic": traffic,
                # SURVEY 8d definition (B): compulsory bytes with a perfect cache - own state read + written (1,024 B) and 4 B of ids per edge
                "traffic_over_compulsory": (traffic / ((1024.0 + 4.0 * nn_max) * n1)) if traffic else None,
                "avg_launch_ms": dom["avg_launch_ms"], "atoms_per_launch": n1,
                "hbm": {"algorithmic_bytes_per_launch": b_a, "achieved_GBps": b_a / t_s / 1e9, "peak_GBps": PEAK_HBM_GBS, "frac": hbm_frac,
                        "definition": "SURVEY 8d (A): gather-counted bytes, (1,024 + 532 nn) per atom-layer - own state read + written (the "
                                      "kernel does both) and, per edge, the neighbour's 512 B state, 16 B geometry and 4 B id. The launch is the "
                                      "whole layer since round 2 (in round 1 a 23-29 us node launch per layer was timed separately and not "
                                      "counted in this kernel's duration). Most gathers hit L2 / Infinity Cache, so this is a cache-bandwidth figure priced at "
                                      "the HBM peak; `traffic` is what actually reached the fabric"},
                "mfma": {"executed_flops_per_launch": f_exec, "achieved_TFLOPs": f_exec / t_s / 1e12, "peak_TFLOPs": PEAK_F16_TFLOPS, "frac": mfma_frac,
                         "definition": "FLOPs the matrix cores execute (3 products per f16-split GEMM, fp32 accumulate) / dense f16 MFMA peak "
                                       "(spec 2.5 PF; v_mfma_f32_16x16x32_f16 itself tops out at 2.0-2.1 PF on this chip, "
                                       "profiles/microbench/r02_peaks.txt)"},
                "useful_TFLOPs": f_ref / t_s / 1e12,
                "useful_definition": "reference-formulation FLOPs of the edge part (SURVEY 8d: 2 x 36,376 x nn per atom) / time; the kernel executes "
                                     "fewer (first-layer linearity) on the f16 pipe, so this is NOT a fraction of any peak",
                "traffic_note": traffic_note,
                # every layer kernel, not only the dominant one: the worst fraction is visible in the line
                "per_nn": per_nn,
            }
        whole = {"layers_ms": layers_ms, "forward_ms": fwd_ms, "launches": n_launch,
                 "forward_ms_p10_p90": [float(np.percentile(fwd_all, 10)), float(np.percentile(fwd_all, 90))],
                 "hbm_frac_def_A": gbytes / (layers_ms * 1e-3) / 1e9 / PEAK_HBM_GBS, "bytes_def_A_per_forward": gbytes,
                 "executed_mfma_frac_of_f16_peak": executed_mfma_flops(config, n1) / (layers_ms * 1e-3) / 1e12 / PEAK_F16_TFLOPS,
                 "useful_TFLOPs": flops / (layers_ms * 1e-3) / 1e12,
                 "hbm_bytes_per_forward_measured": traffic_file.get("hbm_bytes_per_forward") if traffic_file else None,
                 "kernels": kern}

        # ---- side sample: >= 200 consecutive steps, one HIP event pair per step on the launch stream (no host sync in between)
        if not args.no_extras:
            n_long = max(200, args.steps)
            evs = [torch.cuda.Event(enable_timing=True) for _ in range(n_long + 1)]
            # the clock and the package power THIS box holds under the workload (the stamped roofline.clock_GHz is the profile box's): amdsmi's
            # current gfx clock / socket power through torch, sampled by a host thread while the 200 steps run (boxes of the pool differ by
            # several per cent in the clock they hold at the 1,400 W cap - VERDICT r5 weak item 4)
            import threading
            live, stop = [], threading.Event()

            def sampler():
                while not stop.is_set():
                    try:
                        live.append((float(torch.cuda.clock_rate(dev)), float(torch.cuda.power_draw(dev))))
                    except Exception:      # noqa: BLE001 - no amdsmi on this host: the keys stay null
                        return
                    time.sleep(0.004)
            th = threading.Thread(target=sampler, daemon=True)
            barrier()
            th.start()
            evs[0].record()
            for i in range(n_long):
                step()
                evs[i + 1].record()
            torch.cuda.synchronize()
            stop.set()
            th.join(timeout=2.0)
            dt = np.array([evs[i].elapsed_time(evs[i + 1]) for i in range(n_long)])
            live_clock = None
            if len(live) >= 8:
                lv = np.array(live[len(live) // 4:])      # (the first quarter: the queue is still filling)
                pw = lv[:, 1] / (1000.0 if np.median(lv[:, 1]) > 5000.0 else 1.0)
                live_clock = {"sclk_GHz_mean": float(lv[:, 0].mean() / 1e3), "sclk_GHz_min_max": [float(lv[:, 0].min() / 1e3), float(lv[:, 0].max() / 1e3)],
                              "power_W_mean": float(pw.mean()), "samples": int(len(lv)),
                              "how": "torch.cuda.clock_rate() / power_draw() (amdsmi) every 4 ms from a host thread during the 200-step sample; the mean "
                                     "over the forward's kernel mix (k_edge<64> holds less, k_edge<8> more)"}
            long_sample = {"steps": n_long, "ms_per_step_median": float(np.median(dt)), "ms_per_step_p10": float(np.percentile(dt, 10)),
                           "ms_per_step_p90": float(np.percentile(dt, 90)), "ms_per_step_mean": float(dt.mean()),
                           "structures_per_s_from_median": args.batch / float(np.median(dt)) * 1e3, "live_clock": live_clock,
                           "how": "HIP events between consecutive steps on torch's current stream (the stream the kernels are launched on)"}

        # ---- the same forward with the mask pre-reduced by the caller (forward_segments: res_of_atom instead of M); until round 5 the headline
        if not args.no_extras:
            n_sig = max(5, min(args.steps, 20))
            for _ in range(2):
                zs = step_segments()
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            for _ in range(n_sig):
                zs = step_segments()
            torch.cuda.synchronize()
            t_sig = (time.perf_counter() - t1) / n_sig
            seg_call = {"call": "Model.forward_segments(X, ids_topk, q, res_of_atom, R): the dense mask reduced by the caller (not in the timed region)",
                        "mask_bytes_not_read": int(n_atoms_total) * int(R) * 4, "steps": n_sig, "ms_per_step": t_sig * 1e3,
                        "structures_per_s": args.batch / t_sig, "bitwise_equal_to_the_headline_call": bool(torch.equal(zs, z)),
                        "step_minus_this_step_ms": elapsed / args.steps * 1e3 - t_sig * 1e3}
            # the mask pass by itself: HIP events around n_sig reductions of the resident mask on the stream the forward runs on (the difference of
            # the two timed legs above is smaller than their run-to-run spread)
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
            model._segments(Md)
            torch.cuda.synchronize()
            ev[0].record()
            for _ in range(n_sig):
                model._segments(Md)
            ev[1].record()
            torch.cuda.synchronize()
            seg_call["mask_pass_ms_per_step"] = ev[0].elapsed_time(ev[1]) / n_sig
            seg_call["mask_pass_GBps"] = int(n_atoms_total) * int(R) * 4 / (seg_call["mask_pass_ms_per_step"] * 1e-3) / 1e9

        # ---- side measurement: batch-1 latency (ms per structure when structures arrive one at a time)
        if not args.no_latency and args.batch > 1:
            X1, ids1, q1, roa1, R1 = make_batch(args.atoms, 1, 1000 * rank + 1, n0, args.order)
            a = [torch.from_numpy(v).to(dev) for v in (X1, ids1, q1, roa1)]
            def calls(n):
                t1 = time.perf_counter()
                for _ in range(n):
                    model.forward_segments(a[0], a[1], a[2], a[3], R1)
                torch.cuda.synchronize()
                return (time.perf_counter() - t1) / n * 1e3
            calls(3)
            # a burst on an idle GPU: its first ten calls (what rounds 1 - 4 reported as ms_per_structure_batch1: 3 warm-up calls, 10 timed)
            time.sleep(0.1)
            lat_cold = calls(10)
            # steady state of back-to-back calls: the clocks have ramped (about 30 calls, profiles/r05_clock_ramp.txt)
            calls(30)
            lat_ms = calls(50)
            lat_detail = {"steady_state_ms": lat_ms, "calls": 50, "warmup_calls": 43,
                          "first_10_calls_after_100ms_idle_ms": lat_cold,
                          "note": "one model.forward_segments call per structure on device tensors, precision as the line; the GPU drops to its idle "
                                  "clocks within tens of ms without work and needs ~30 calls to ramp back (profiles/r05_clock_ramp.txt)"}

    # ---- BASELINE config 4 as a strong-scaling leg (every world size runs the same list)
    stage[0] = "config-4 legs (sharding.forward_sharded)"
    cfg4 = cfg4_dense = cfg4_strong = None
    if ((args.full and not args.no_extras) or args.mode == "strong") and args.config == "i_v4_1":
        # (--mode strong: this leg is the headline - its gathered logits are what --dump-outputs writes besides z)
        cfg4_out = {} if args.mode == "strong" and args.dump_outputs else None
        cfg4 = config4_leg(model, dist, args.backend, dev, args.config4_structures * world, max(3, min(args.steps, 5)), args.config4_max_atoms,
                           outputs=cfg4_out)
        if cfg4_out:
            dump_outputs(args.dump_outputs, cfg4_out)
        if args.full:
            # the same list in the reference loader's OWN per-structure forms (dense one-hot q, bool M, int64 ids): every reduction inside the
            # timed region (ADVICE r4 / VERDICT r4 item 6: the compact leg above pre-reduces outside it)
            cfg4_dense = config4_leg(model, dist, args.backend, dev, args.config4_structures * world, 3, args.config4_max_atoms, forms="dense")
            if world > 1:
                # SURVEY 8e's acceptance is about a FIXED list (>= 7x on 8 GPUs, >= 64 structures): the same 512 structures at every world
                # size, with the world-1 time of that list taken on rank 0 inside this run
                cfg4_strong = config4_leg(model, dist, args.backend, dev, args.strong_structures, 3, args.config4_max_atoms, fixed_list=True)
        if rank == 0 and cfg4 is not None:
            cfg4["dense_forms"] = cfg4_dense

    if rank == 0:
        n_struct = args.steps * args.batch * world
        weak_value = n_struct / elapsed
        strong = args.mode == "strong" and cfg4 is not None
        out = {
            "metric": "structures/sec (N=3000 atoms, k=64, 32 layers)" if args.config == "i_v4_1" and args.atoms == 3000 and not strong
                      else ("structures/sec (i_v4_1, fixed list of pdbs_test-sized structures, sharded)" if strong
                            else f"structures/sec ({args.config}, N={args.atoms})"),
            "value": cfg4["value"] if strong else weak_value,
            "unit": "structures/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "full": bool(args.full),
            "ms_per_step": elapsed / args.steps * 1e3,
            "ms_per_structure": elapsed / n_struct * 1e3,
            "ms_per_structure_batch1": lat_ms,
            "batch1": lat_detail,
            "preroll": {"ms": args.preroll_ms, "steps": preroll_steps,
                        "why": "untimed steps in front of the W warm-up steps: the host-side set-up leaves the GPU idle, and an idle MI355X needs "
                               "~30 ms of work to reach its steady clocks"},
            "long_sample": long_sample,
            "segment_call": seg_call,
            "higher_is_better": True,
            "scaling": "strong" if strong else "weak",
            "vs_baseline": None,
            "dtype": {"auto": "f32 (3xf16-split MFMA, fp32 accumulate; fp32 re-run on f16-range overflow)",
                      "f16_split": "f32 (3xf16-split MFMA, fp32 accumulate)", "fp32": "f32 (exact fp32 MFMA)"}[args.precision],
            "data": "synthetic",
            "config": {"workload": (cfg4["workload"] if strong else
                                    f"{args.config} Model.forward(X, ids_topk, q, M) ({len(config['sum'])} state-update layers), synthetic cloud "
                                    f"N={args.atoms} atoms k=64 R={R // args.batch} per structure, {args.batch} structures "
                                    f"collated per step per GPU (dense fp32 mask M [{n_atoms_total}, {R}] = {n_atoms_total * R * 4 / 1e6:.0f} MB read and "
                                    f"reduced on the GPU inside every step), atom order {args.order}, inputs resident in HBM, {wdesc}"),
                       "call": "Model.forward(X, ids_topk, q, M)", "mask_bytes_per_step": int(n_atoms_total) * int(R) * 4,
                       "atoms_per_step_per_gpu": int(n_atoms_total), "structures_per_step_per_gpu": args.batch,
                       "precision": args.precision, "fp32_reruns_in_timed_region": status["n_fp32_rerun"],
                       "sharding": f"{world} rank(s), independent structures per rank, no data-path collective"},
            "weak_value": weak_value,
            # N > 1: every rank's own time for the same number of steps (a separate pass right behind the timed one) - a straggling GPU
            # or rank is visible here, the headline takes the max over ranks
            "per_rank": None if rank_times is None else [{"rank": r_, "seconds": t_, "value": args.steps * args.batch / t_} for r_, t_ in enumerate(rank_times)],
            "rank_time_max_over_min": None if rank_times is None else max(rank_times) / min(rank_times),
            "value_exact_fp32": exact["value"] if exact else None,
            "exact_fp32": exact,
            "exact_fp32_max_abs_vs_timed_output": exact["max_abs_vs_timed_output"] if exact else None,
            "parity_max_abs": parity,
            "parity_note": "max |z - reference golden| over structure 0 of the LAST timed step (tests/golden/fwd_i_v4_1_stacked_synth3000.npz, "
                           "reference PyTorch CPU output); asserted < 1e-4" if parity is not None else None,
            "roofline": roofline,
            "whole_forward": whole,
            "config4_sharded": cfg4,
            "config4_strong": cfg4_strong,
            # what the collective library saw: ranks counted by an all_reduce of ones (device tensors under nccl = RCCL), the device of every
            # rank, and the weight broadcast every handle was built from
            "rccl_ranks_seen": ranks_info["ranks_seen"], "ranks": ranks_info, "weights_broadcast": wb,
        }
        if args.full and args.cpu_budget > 0 and world == 1:      # the CPU baseline is a 1-GPU-run side measurement (rank 0, N = 1 only)
            key = {"i_v4_1": "2:", "i_v3_0": "3:"}.get(args.config, "2:")
            out["cpu_baseline"] = cpu_baseline(config, sd, args.atoms, args.cpu_budget, key)
            out["speedup_vs_cpu_baseline"] = out["value"] / out["cpu_baseline"]["value"]
            if out["cpu_baseline"].get("reference_equivalent"):
                # an ESTIMATE: rho (reference / port) was measured on another machine - the build container, 8 threads
                # (profiles/r06_cpu_rho.json) - and multiplies the port's time at 8 threads on this host
                out["speedup_vs_reference_equivalent_cpu_estimate"] = out["value"] / out["cpu_baseline"]["reference_equivalent"]["structures_per_s"]
        print(json.dumps(out), flush=True)
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
