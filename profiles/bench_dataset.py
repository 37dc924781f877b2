"""Dataset build rates (pesto_amd.dataset) on the tree's PDB assemblies and synthetic ones.

    python profiles/bench_dataset.py [--copies 8] [--out profiles/r08_dataset.txt]

Reports assemblies per second of build_dataset end to end, the time by stage measured separately on the same inputs (read + preprocess on
host threads, contacts + typed keys, k-NN, HDF5 write), and the contacts + types stage against the reference's dense method restated in
torch on the same GPU (one torch.norm distance matrix per pair of subunits, torch.where, a dense [R0, R1, 79, 79] map per pair).
"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from pesto_amd import Model, dataset  # noqa: E402
from pesto_amd.config import CONFIGS  # noqa: E402

CASES = ["1H9D", "1OL5", "1ZNS", "6O1T", "3IVK", "7KHT"]


def synthetic(k, n_sub=40, n=150, seed=0):
    rng = np.random.default_rng(seed + k)
    subs = {}
    for s in range(n_sub):
        c = rng.uniform(0, 45, 3)
        res = np.repeat(np.arange(n // 6), 6)
        subs[f"S{s:02d}"] = {"xyz": (c + rng.normal(0, 4.0, (n, 3))).astype(np.float32), "resid": res,
                             "resname": np.array([dataset.MOLECULE_IDS[(s + r) % 30] for r in res])}
    return subs


def dense_reference(subunits, mids, dev, r_thr=5.0):
    """extract_all_contacts + contacts_types restated in torch on the GPU (the reference's dense method)."""
    names = list(subunits)
    X = {c: torch.from_numpy(np.asarray(subunits[c]["xyz"], np.float32)).to(dev) for c in names}
    enc = {}
    for c in names:
        _, res = np.unique(subunits[c]["resid"], return_inverse=True)
        M = torch.zeros((res.size, int(res.max()) + 1), dtype=torch.bool, device=dev)
        M[torch.arange(res.size), torch.from_numpy(res.reshape(-1)).to(dev)] = True
        oh = torch.from_numpy(np.asarray(subunits[c]["resname"]).reshape(-1, 1) == mids.reshape(1, -1)).to(dev)
        enc[c] = (M, oh)
    n = 0
    for i in range(len(names)):
        for j in range(i + 1, len(names)):
            D = torch.norm(X[names[i]].unsqueeze(1) - X[names[j]].unsqueeze(0), dim=2)
            a, b = torch.where(D < r_thr)
            if a.shape[0] == 0:
                continue
            M0, c0 = enc[names[i]]
            M1, c1 = enc[names[j]]
            H = c1[b].unsqueeze(1) & c0[a].unsqueeze(2)
            Y = torch.zeros((M0.shape[1], M1.shape[1], H.shape[1], H.shape[2]), device=dev, dtype=torch.bool)
            Y[torch.where(M0[a])[1], torch.where(M1[b])[1]] = H
            if torch.any(Y):
                torch.stack(torch.where(Y), dim=1)
                torch.stack(torch.where(Y.permute(1, 0, 3, 2)), dim=1)
            n += 1
    torch.cuda.synchronize(dev)
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--copies", type=int, default=8)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    model = Model(CONFIGS["i_v4_0"]).to(dev)
    from pesto_amd.weights import blob_size
    model.load_blob(np.zeros(blob_size(model.config), np.float32))
    tmp = tempfile.mkdtemp()
    lines = []

    def log(s):
        print(s, flush=True)
        lines.append(s)

    try:
        paths = []
        for k in range(args.copies):
            for c in CASES:
                p = os.path.join(tmp, f"{c.lower()}{k}.pdb1.gz")
                shutil.copy(os.path.join(ROOT, "tests", "golden", "pdb", f"{c}.pdb1.gz"), p)
                paths.append(p)
        key_of = lambda p: (os.path.basename(p).split(".")[0], "1")  # noqa: E731
        dataset.build_dataset(model, paths[:len(CASES)], os.path.join(tmp, "warm.h5"), key_of=key_of, on_error=None)     # warm-up
        t0 = time.perf_counter()
        summ = dataset.build_dataset(model, paths, os.path.join(tmp, "out.h5"), key_of=key_of, on_error=None)
        t_e2e = time.perf_counter() - t0
        log(f"build_dataset end to end: {len(paths)} assemblies ({args.copies} copies of {len(CASES)} PDB assemblies) in {t_e2e:.3f} s "
            f"= {len(paths) / t_e2e:.1f} assemblies/s; {summ['structures']} structure groups, {summ['contacts']} contact groups")
        # stages, measured one at a time on the same inputs
        from concurrent.futures import ThreadPoolExecutor
        t0 = time.perf_counter()
        with ThreadPoolExecutor(8) as ex:
            read = list(ex.map(lambda p: dataset._read_assembly(p, key_of, dataset.MAX_NUM_ATOMS), paths))
        t_read = time.perf_counter() - t0
        asm = [(k, s) for st, k, s in read if st == "ok"]
        rows = [dataset._subunit_rows(s, dataset.MOLECULE_IDS) for _, s in asm]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out, meta = dataset._contacts_call(model, rows, 5.0, dataset.MOLECULE_IDS, False)
        torch.cuda.synchronize()
        t_ct = time.perf_counter() - t0
        contacts = dataset._contact_dicts(out, meta)
        typed = dataset._typed_items(out, meta, [{r[0]: r[4] for r in rw} for rw in rows], len(dataset.MOLECULE_IDS))
        Xs = [np.asarray(s[c]["xyz"], np.float32) for (_, s), ct in zip(asm, contacts) for c in ct]
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        model.knn_collate(np.concatenate(Xs), [x.shape[0] for x in Xs])
        t_knn = time.perf_counter() - t0
        t0 = time.perf_counter()
        items = []
        for (key, s), ct, ty in zip(asm, contacts, typed):
            st = dataset._structure_items(model, [(c, s[c]) for c in ct], 64)
            items.append((key, *dataset._pack(ct, ty, st)))
        t_pack = time.perf_counter() - t0
        from pesto_amd.h5store import H5Store
        t0 = time.perf_counter()
        with H5Store(os.path.join(tmp, "w.h5"), "w") as hf:
            for key, sd, cd in items:
                dataset._write_items(hf, key, sd, cd, None)
        t_h5 = time.perf_counter() - t0
        log(f"stages (separately, {len(asm)} assemblies): read + preprocess {t_read * 1e3:.1f} ms (8 threads); contacts + types "
            f"{t_ct * 1e3:.2f} ms (one launch sequence, host pointers); k-NN {t_knn * 1e3:.2f} ms ({len(Xs)} subunits, one call); "
            f"encode + pack (incl. k-NN) {t_pack * 1e3:.1f} ms; HDF5 write {t_h5 * 1e3:.1f} ms")
        # contacts + types: this library vs the dense torch method, PDB assemblies and synthetic ones
        for label, subs_list in (("PDB", [s for _, s in asm[:len(CASES)]]), ("synthetic 40 x 150 atoms", [synthetic(k) for k in range(4)])):
            rows = [dataset._subunit_rows(s, dataset.MOLECULE_IDS) for s in subs_list]
            dataset._contacts_call(model, rows, 5.0, dataset.MOLECULE_IDS, False)
            reps = 5
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                dataset._contacts_call(model, rows, 5.0, dataset.MOLECULE_IDS, False)
            torch.cuda.synchronize()
            t_hip = (time.perf_counter() - t0) / reps
            dense_reference(subs_list[0], dataset.MOLECULE_IDS, dev)
            t0 = time.perf_counter()
            for _ in range(reps):
                for s in subs_list:
                    dense_reference(s, dataset.MOLECULE_IDS, dev)
            t_ref = (time.perf_counter() - t0) / reps
            log(f"contacts + types, {len(subs_list)} {label} assemblies: pesto_contacts {t_hip * 1e3:.2f} ms "
                f"({len(subs_list) / t_hip:.0f} assemblies/s), dense torch restatement {t_ref * 1e3:.1f} ms "
                f"({len(subs_list) / t_ref:.1f} assemblies/s): {t_ref / t_hip:.1f}x")
    finally:
        shutil.rmtree(tmp, ignore_errors=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("# profiles/bench_dataset.py on one MI355X (gfx950)\n" + "\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
