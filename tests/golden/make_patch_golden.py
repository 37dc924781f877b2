#!/usr/bin/env python3
"""Generate the interface-patch golden (tests/golden/patches.npz) by IMPORTING the reference's own cluster_interfaces (interfaceome/
cluster_interfaces.py), cluster_multi_interfaces and follow_rabbits (interfaceome/cluster_multi_interfaces.py) from /root/reference (build
container only; nothing under tests/ reads the reference at run time). h5py, tqdm and structures_store are stubbed: none is called.

Cases (each a batch of structures, rows = residue rows of p):
  pdbs53    the 53 pdbs_test chains: CA rows located with the native reader (Structure.encode numbering), p = sigmoid(z_i_v4_0) of
            cfg4_all53.npz, a deterministic synthetic afs; threshold sets (70, 0.5, 10.0) and (50.5, 0.3, 6.5)
  examples  the 7 examples/ complexes of examples_complexes.npz with p from their _i0.._i4 b-factor files (2 decimals: many values are
            exactly 0.50); residues without a CA (nucleotides, ions, ligands) are never nodes; no afs (the reference gets afs = 100)
  synth     pairs planted at exactly d_thr ((0,0,0)-(6,8,0), (0,0,0)-(10,0,0)) and one float32 ulp either side, R = 1, a structure with
            nothing selected, NaN afs
  big       a 20,000-residue helix (3.8 A steps): one path-like patch in the protein selection, every other selection empty
The reference runs on the CA rows (its entry has one row per CA); its patch members are mapped back to residue rows. Stored per case
and threshold set t: the inputs (<case>_offsets, _xyz, _p, _afs, _has_ca) and, for both reference functions (form "multi": the 15 keys of
cluster_multi_interfaces, "single": the 5 lists of cluster_interfaces), <case>_t<t>_<form>_npatch [S, n_sel], _len [patches] and
_members [rows] - the patches in the reference's order, members ascending.

Usage:  python tests/golden/make_patch_golden.py
"""
import os
import sys
import types

import numpy as np

REF = "/root/reference"
OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
EXAMPLE_DIRS = {"1ZNS": "endonuclease", "7KHT_lipid": "lipids", "3IVK": "dna_rna", "1H9D": "dna_rna", "6O1T": "lipids", "6XRU": "lipids",
                "6Y5B": "channel"}
THRESHOLDS = {"pdbs53": [(70.0, 0.5, 10.0), (50.5, 0.3, 6.5)], "examples": [(70.0, 0.5, 10.0), (50.5, 0.3, 6.5)],
              "synth": [(70.0, 0.5, 10.0)], "big": [(70.0, 0.5, 10.0)]}


def import_reference():
    for name in ("h5py", "tqdm"):
        if name not in sys.modules:
            try:
                __import__(name)
            except ImportError:
                sys.modules[name] = types.ModuleType(name)
    if not hasattr(sys.modules["tqdm"], "tqdm"):
        sys.modules["tqdm"].tqdm = lambda x, *a, **k: x
    ss = types.ModuleType("structures_store")
    ss.h5_load_structure = lambda hf: None
    sys.modules["structures_store"] = ss
    sys.path.insert(0, os.path.join(REF, "interfaceome"))
    import cluster_interfaces
    import cluster_multi_interfaces
    return cluster_interfaces, cluster_multi_interfaces


def reference_patches(ci, cmi, xyz, p, afs, has_ca, thr):
    """(multi: [15][patches][members], single: [5][patches][members]) of one structure, in residue rows"""
    ca = np.nonzero(has_ca)[0]
    entry = {"x": xyz[ca, 0], "y": xyz[ca, 1], "z": xyz[ca, 2], "afs": (afs if afs is not None else np.full(len(p), 100.0, np.float32))[ca]}
    for c in range(5):
        entry[f"p{c}"] = p[ca, c]
    multi = cmi.cluster_interfaces(entry, *thr)
    single = ci.cluster_interfaces(entry, *thr)
    keys = [ci_ if ci_ == cj else f"{ci_}+{cj}" for a, ci_ in enumerate(LABELS) for cj in LABELS[a:]]
    assert list(multi) == keys
    back = lambda pl: [sorted(int(ca[v]) for v in m) for m in pl]
    multi = [back(multi[k]) for k in keys]
    single = [back(v) for v in single]
    for pl in multi + single:
        assert [m[0] for m in pl] == sorted(m[0] for m in pl)        # follow_rabbits' order: by the smallest member
    for i in range(5):
        assert single[i] == multi[keys.index(LABELS[i])]
    return multi, single


LABELS = ["protein", "dna/rna", "ion", "ligand", "lipid"]


def flatten(per_struct):
    npatch = np.array([[len(pl) for pl in sel] for sel in per_struct], np.int32)
    lens = [len(m) for sel in per_struct for pl in sel for m in pl]
    mem = [v for sel in per_struct for pl in sel for m in pl for v in m]
    return npatch, np.array(lens, np.int32), np.array(mem, np.int32)


def case_pdbs53():
    from pesto_amd.patches import residue_ca
    from pesto_amd.structure_io import Structure
    g = np.load(os.path.join(OUT, "cfg4_all53.npz"))
    offs = g["res_offsets"].astype(np.int32)
    z = g["z_i_v4_0"].astype(np.float32)
    p = (1.0 / (1.0 + np.exp(-z.astype(np.float64)))).astype(np.float32)
    xyz, has = [], []
    for s, name in enumerate(g["names"].astype(str)):
        st = Structure.read_pdb(os.path.join(REF, "pdbs_test", name + ".pdb")).preprocess()
        x, h, _ = residue_ca(st)
        assert x.shape[0] == offs[s + 1] - offs[s], name
        xyz.append(x); has.append(h)
    R = int(offs[-1])
    afs = (40.0 + 0.5 * np.random.default_rng(53).integers(0, 121, R)).astype(np.float32)      # 40.0 .. 100.0 in 0.5 steps: 50.5 and 70.0 occur
    return offs, np.concatenate(xyz), p, afs, np.concatenate(has)


def case_examples():
    from pesto_amd.patches import residue_ca
    from pesto_amd.structure_io import Structure
    g = np.load(os.path.join(OUT, "examples_complexes.npz"))
    offs = g["res_offsets"].astype(np.int32)
    xyz, has, ps = [], [], []
    for s, name in enumerate(g["names"].astype(str)):
        d = os.path.join(REF, "examples", EXAMPLE_DIRS[name])
        st = Structure.read_pdb(os.path.join(d, name + ".pdb")).preprocess()
        x, h, _ = residue_ca(st)
        R = offs[s + 1] - offs[s]
        assert x.shape[0] == R, name
        p = np.zeros((R, 5), np.float32)
        for c in range(5):
            sc = Structure.read_pdb(os.path.join(d, f"{name}_i{c}.pdb")).preprocess()
            _, _, roa, Rc = sc.encode(30)
            assert Rc == R, (name, c)
            bf = sc.bfactor()
            first = np.full(R, -1)
            first[roa[::-1]] = np.arange(len(roa))[::-1]
            p[:, c] = bf[first]
            assert np.array_equal(bf, p[roa, c])            # one value per residue
        xyz.append(x); has.append(h); ps.append(p)
    return offs, np.concatenate(xyz), np.concatenate(ps), None, np.concatenate(has)


def case_synth():
    f = np.float32
    up, dn = lambda v: np.nextafter(f(v), f(np.inf)), lambda v: np.nextafter(f(v), f(-np.inf))
    structs = []
    # planted distances around d_thr = 10: groups 100 A apart, each a pair
    pairs = [((0, 0, 0), (6, 8, 0)), ((0, 0, 0), (up(6), 8, 0)), ((0, 0, 0), (dn(6), 8, 0)), ((0, 0, 0), (10, 0, 0)),
             ((0, 0, 0), (dn(10), 0, 0)), ((0, 0, 0), (up(10), 0, 0)), ((0, 0, 0), (0, 0, dn(dn(10)))), ((1.5, -2.25, 3), (7.5, 5.75, 3))]
    # pairs 100 A apart along an axis on which both points of the pair share the coordinate (the offset leaves their difference exact)
    shift = lambda k, pr: (100 * k, 0, 0) if pr[0][2] != pr[1][2] else (0, 0, 100 * k)
    x = np.array([np.add(q, shift(k, pr)) for k, pr in enumerate(pairs) for q in pr], np.float32)
    n = len(x)
    p = np.full((n, 5), 0.9, np.float32)
    p[:, 2] = 0.5                                   # exactly p_thr: never a node
    p[::2, 3] = up(0.5)                             # one ulp above: a node
    p[1::2, 3] = 0.1
    structs.append((x, p, np.full(n, 90, np.float32), np.ones(n, np.uint8)))
    # R = 1
    structs.append((np.zeros((1, 3), np.float32), np.full((1, 5), 0.9, np.float32), np.full(1, 90, np.float32), np.ones(1, np.uint8)))
    # nothing selected (p below, afs below, no CA)
    rng = np.random.default_rng(5)
    x = (rng.standard_normal((300, 3)) * 8).astype(np.float32)
    p = rng.uniform(0, 1, (300, 5)).astype(np.float32)
    p[:100] = 0.2
    afs = np.full(300, 90, np.float32)
    afs[100:200] = 70.0                             # exactly afs_thr: never a node
    has = np.ones(300, np.uint8)
    has[200:] = 0
    structs.append((x, p, afs, has))
    # NaN afs and NaN p on a dense random cloud
    x = (rng.standard_normal((800, 3)) * 12).astype(np.float32)
    p = rng.uniform(0.3, 1, (800, 5)).astype(np.float32)
    p[rng.integers(0, 800, 40), rng.integers(0, 5, 40)] = np.nan
    afs = rng.uniform(60, 100, 800).astype(np.float32)
    afs[rng.integers(0, 800, 60)] = np.nan
    structs.append((x, p, afs, np.ones(800, np.uint8)))
    offs = np.cumsum([0] + [len(s[0]) for s in structs]).astype(np.int32)
    return offs, np.concatenate([s[0] for s in structs]), np.concatenate([s[1] for s in structs]), \
        np.concatenate([s[2] for s in structs]), np.concatenate([s[3] for s in structs])


def big_helix(n=20000):
    """CA-like helix: radius 2.3 A, 100 degrees and 1.5 A rise per residue (3.8 A steps); coordinates rounded to 1/256 A"""
    t = np.arange(n) * np.deg2rad(100.0)
    x = np.stack([2.3 * np.cos(t), 2.3 * np.sin(t), 1.5 * np.arange(n) - 15000.0], 1)
    return (np.round(x * 256) / 256).astype(np.float32)


def case_big():
    x = big_helix()
    n = len(x)
    p = np.full((n, 5), 0.1, np.float32)
    p[:, 0] = 0.9
    return np.array([0, n], np.int32), x, p, np.full(n, 90, np.float32), np.ones(n, np.uint8)


def main():
    ci, cmi = import_reference()
    out = {}
    for case, fn in (("synth", case_synth), ("examples", case_examples), ("pdbs53", case_pdbs53), ("big", case_big)):
        offs, xyz, p, afs, has = fn()
        out[f"{case}_offsets"], out[f"{case}_p"], out[f"{case}_has_ca"] = offs, p, has
        if case == "big":
            out[f"{case}_xyz256"] = np.round(xyz.astype(np.float64) * 256).astype(np.int32)     # exact: xyz = xyz256 / 256
        else:
            out[f"{case}_xyz"] = xyz
        if afs is not None:
            out[f"{case}_afs"] = afs
        for t, thr in enumerate(THRESHOLDS[case]):
            multi, single = [], []
            for s in range(len(offs) - 1):
                r0, r1 = offs[s], offs[s + 1]
                m, sg = reference_patches(ci, cmi, xyz[r0:r1], p[r0:r1], None if afs is None else afs[r0:r1], has[r0:r1], thr)
                multi.append(m); single.append(sg)
            out[f"{case}_t{t}_thr"] = np.array(thr, np.float64)
            for form, v in (("multi", multi), ("single", single)):
                npatch, lens, mem = flatten(v)
                out[f"{case}_t{t}_{form}_npatch"], out[f"{case}_t{t}_{form}_len"], out[f"{case}_t{t}_{form}_members"] = npatch, lens, mem
            print(f"{case} t{t}: {len(offs) - 1} structures, {int(offs[-1])} rows, {int(out[f'{case}_t{t}_multi_npatch'].sum())} patches "
                  f"(multi), largest {int(out[f'{case}_t{t}_multi_len'].max(initial=0))}", flush=True)
    out["cases"] = np.array(["pdbs53", "examples", "synth", "big"])
    path = os.path.join(OUT, "patches.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
