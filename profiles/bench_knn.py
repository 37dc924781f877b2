#!/usr/bin/env python3
"""Timing of the GPU k-NN topology + collate kernel beside the host path it replaces.
usage: python profiles/bench_knn.py   (on the GPU box; prints one JSON line per case)"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from pesto_amd import Model
from pesto_amd.config import CONFIGS
from pesto_amd.topology import collate_batch_features, extract_topology, synthetic_cloud
from pesto_amd.weights import synthetic_state_dict

m = Model(CONFIGS["i_v4_0"]).to("cuda:0")
m.load_state_dict(synthetic_state_dict(CONFIGS["i_v4_0"]))
for name, sizes in (("8 x N=3000 (bench batch)", [3000] * 8), ("1 x N=20000 (config 5)", [20000]), ("53 chains, N 1641-3052", list(np.random.default_rng(0).integers(1641, 3053, 53))),
                    ("sparse cube 250 A, N=20000", [20000])):
    Xs = [synthetic_cloud(int(n), 7 + i) for i, n in enumerate(sizes)]
    if name.startswith("sparse"):       # uniform over a 250 A cube: the cell cap of pesto_cellgrid.h binds, most cells are empty
        Xs = [np.random.default_rng(5).uniform(0, 250, (sizes[0], 3)).astype(np.float32)]
    X = np.concatenate(Xs)
    Xd = torch.from_numpy(X).cuda()
    for _ in range(3):
        ids = m.knn_collate(Xd, sizes)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    reps = 20
    for _ in range(reps):
        ids = m.knn_collate(Xd, sizes)
    torch.cuda.synchronize()
    t_gpu = (time.perf_counter() - t0) / reps
    # host path of the reference contract (numpy: dense O(N^2) below 4096 atoms, k-d tree above), one structure at a time
    t0 = time.perf_counter()
    batch = [[x, extract_topology(x, 64), np.zeros((x.shape[0], 1), np.float32), np.ones((x.shape[0], 1), bool)] for x in Xs[:8]]
    collate_batch_features(batch)
    t_host = (time.perf_counter() - t0) * len(Xs) / min(len(Xs), 8)
    pairs = float(sum(int(n) ** 2 for n in sizes))
    print(json.dumps({"case": name, "atoms": int(X.shape[0]), "gpu_ms": t_gpu * 1e3, "gpu_pair_distances_per_s": pairs / t_gpu,
                      "host_numpy_ms": t_host * 1e3, "speedup": t_host / t_gpu}))
