#!/usr/bin/env python3
"""Generate the solvent-accessible-surface-area golden (tests/golden/sasa.npz) from a NumPy float32 restatement of the definition in
pesto_amd/sasa.py (mdtraj is not available, so its output cannot be recorded; the definition is the contract). Everything runs on the CPU.

The restatement (exposed_counts): per atom, the points t = X_i + (R_i * S) and, against every candidate j, q = (dx*dx + dy*dy) + dz*dz
in float32 array operations, each rounded on its own; a point is buried when q < R_j * R_j for some j. Candidates are the finite atoms
j != i of the structure with |X_i - X_j| < |R_i| + |R_j| + margin in float64; the margin (1e-3 of the radii plus 1e-4 of the coordinate
scale, thousands of times the float32 rounding of t and q) is generous, and every case is computed a second time with twice the margin and
asserted to give the same counts.

Cases
  md       the 29 frames x 2,030 atoms of frames_md_1JTG_uL.npz (referenced, not duplicated); radii from its q_idx through
           pesto_amd.sasa.atomic_radii plus the 1.4 A probe (md_R)
  batch    four structures of tests/golden/pdb read with the project's reader (one with a zinc ion and hetero atoms, one with hydrogens,
           one with a lipid); counts per structure, laid end to end
  dense    synthetic_cloud(1500) with R = 6.0: candidate lists of hundreds of atoms
  planted  two equal spheres (R = 3.1, d = 3.0: 712 of 960 exposed points, analytic 712.26); an occluder at exactly R_i + R_j and one
           float32 step either side; a point whose q equals R_j^2 exactly (P = 1, whose one point is (1, 0, 0)) and one step above;
           coincident atoms; a NaN coordinate and an infinite radius; a single atom; a one-atom structure inside a batch; a 40-atom crop of
           md at P = 1, 64, 960 and 1,000
Stored: counts as uint16, the radii, the planted inputs. Areas are not stored: a test evaluates float32(((c0 * count) * R) * R) in double.

Usage:  python tests/golden/make_sasa_golden.py
"""
import gzip
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(OUT))
sys.path.insert(0, ROOT)
BATCH = ["1thf_D.pdb", "1ZNS_ion.pdb", "6I9F.pdb", "7KHT_lipid_i0.pdb"]
PROBE = np.float32(1.4)


def points(n):
    k = np.arange(n, dtype=np.float64)
    y = k * (2.0 / n) - 1.0 + 1.0 / n
    r = np.sqrt(1.0 - y * y)
    phi = k * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([np.cos(phi) * r, y, np.sin(phi) * r], 1).astype(np.float32)


def exposed_counts(X, R, S, sizes=None, scale=1.0):
    """int [N]: the definition's count of every atom of one frame; scale multiplies the candidate margin"""
    X, R, S = np.asarray(X, np.float32), np.asarray(R, np.float32), np.asarray(S, np.float32)
    N, P = X.shape[0], S.shape[0]
    out = np.full(N, P, np.int64)
    start = 0
    with np.errstate(all="ignore"):
        for n in ([N] if sizes is None else sizes):
            x, r = X[start:start + n], R[start:start + n]
            ok = np.isfinite(x).all(1) & np.isfinite(r)
            x64, r64 = x.astype(np.float64), np.abs(r.astype(np.float64))
            big = float(np.abs(x64[ok]).max()) if ok.any() else 0.0
            r2 = r * r
            for i in np.nonzero(ok)[0]:
                reach = r64[i] + r64 + scale * (1e-3 * (r64[i] + r64) + 1e-4 * (1.0 + big))
                cand = ok & (np.sqrt(((x64 - x64[i]) ** 2).sum(1)) < reach)
                cand[i] = False
                c = np.nonzero(cand)[0]
                if c.size == 0:
                    continue
                t = x[i] + r[i] * S                                   # float32 [P, 3]
                buried = np.zeros(P, bool)
                for c0 in range(0, c.size, 128):
                    cc = c[c0:c0 + 128]
                    d = t[:, None, :] - x[cc][None, :, :]
                    q = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
                    buried |= (q < r2[cc][None, :]).any(1)
                out[start + i] = P - int(buried.sum())
            start += n
    return out


def checked(X, R, S, sizes=None, name=""):
    a = exposed_counts(X, R, S, sizes, 1.0)
    assert np.array_equal(a, exposed_counts(X, R, S, sizes, 2.0)), f"{name}: the counts depend on the candidate margin"
    return a


def main():
    from pesto_amd.sasa import atomic_radii, sphere_points
    from pesto_amd.structure_io import Structure
    from pesto_amd.topology import synthetic_cloud
    out = {}
    S = points(960)
    assert np.array_equal(S, sphere_points(960))
    out["points960"] = S

    # ---- md
    g = np.load(os.path.join(OUT, "frames_md_1JTG_uL.npz"))
    X, R = g["X_frames"], atomic_radii(g["q_idx"][:, 0]) + PROBE
    assert R.dtype == np.float32
    counts = np.stack([checked(X[f], R, S, name=f"md frame {f}") for f in range(X.shape[0])])
    out["md_R"], out["md_counts"] = R, counts.astype(np.uint16)
    area0 = (4.0 * np.pi / 960 * counts[0]) * R.astype(np.float64) * R.astype(np.float64)
    print(f"md frame 0: total {area0.sum():.0f} A^2, {100 * (counts[0] == 0).mean():.0f} % of the atoms fully buried", flush=True)

    # ---- batch
    Xs, Rs = [], []
    for name in BATCH:
        d = Structure.parse_pdb(gzip.open(os.path.join(OUT, "pdb", name + ".gz"), "rb").read()).to_dict()
        Xs.append(d["xyz"])
        Rs.append(atomic_radii(d["element"]) + PROBE)
    sizes = [x.shape[0] for x in Xs]
    assert any((np.asarray(r) == np.float32(1.39) + PROBE).any() for r in Rs)          # the zinc ion
    Xb, Rb = np.concatenate(Xs), np.concatenate(Rs)
    out["batch_names"], out["batch_sizes"], out["batch_R"] = np.array(BATCH), np.array(sizes, np.int32), Rb
    out["batch_counts"] = checked(Xb, Rb, S, sizes, "batch").astype(np.uint16)
    print("batch", sizes, flush=True)

    # ---- dense
    Xd = synthetic_cloud(1500)
    Rd = np.full(1500, 6.0, np.float32)
    out["dense_counts"] = checked(Xd, Rd, S, name="dense").astype(np.uint16)
    print("dense: mean count", out["dense_counts"].mean(), flush=True)

    # ---- planted
    planted = {}

    def plant(name, X, R, P=960, sizes=None):
        X, R = np.asarray(X, np.float32).reshape(-1, 3), np.asarray(R, np.float32).reshape(-1)
        sizes = [X.shape[0]] if sizes is None else sizes
        planted[name] = checked(X, R, points(P), sizes, name)
        out[f"planted_{name}_X"], out[f"planted_{name}_R"], out[f"planted_{name}_P"] = X, R, np.int32(P)
        out[f"planted_{name}_sizes"], out[f"planted_{name}_counts"] = np.array(sizes, np.int32), planted[name].astype(np.uint16)
        return planted[name]

    c = plant("two_spheres", [[0, 0, 0], [0, 3.0, 0]], [3.1, 3.1])
    assert c.tolist() == [712, 712], c
    ri, rj = np.float32(2.0), np.float32(1.5)
    touch = ri + rj
    c = plant("touching", [[0, 0, 0], [np.nextafter(touch, np.float32(0)), 0, 0], [0, 0, 0], [touch, 0, 0], [0, 0, 0],
                           [np.nextafter(touch, np.float32(9)), 0, 0]], [ri, rj] * 3, sizes=[2, 2, 2])
    print("touching", c.tolist())
    # P = 1: the one point is (1, 0, 0), t = (2, 0, 0); the occluder at (5, 0, 0) with R_j = 3 has q = 9 = R_j^2: not buried
    assert points(1).tolist() == [[1.0, 0.0, 0.0]]
    c = plant("q_equals_r2", [[0, 0, 0], [5, 0, 0], [0, 0, 0], [5, 0, 0]], [2.0, 3.0, 2.0, np.nextafter(np.float32(3), np.float32(9))], P=1,
              sizes=[2, 2])
    assert c[0] == 1 and c[2] == 0, c
    c = plant("coincident", [[1, 2, 3], [1, 2, 3], [1, 2, 3], [2.5, 2, 3], [2.5, 2, 3]], [3.0, 3.0, 2.0, 3.0, 3.2])
    print("coincident", c.tolist())
    c = plant("nonfinite", [[0, 0, 0], [np.nan, 1, 0], [2, 0, 0], [1, 1, 1], [0, 2.5, 0], [3, 3, np.inf]], [3.0, 3.0, 3.0, np.inf, 3.0, 3.0])
    assert c[1] == 960 and c[3] == 960 and c[5] == 960 and c[0] < 960, c
    c = plant("single", [[7, -3, 2]], [3.2])
    assert c.tolist() == [960]
    crop = np.argsort(((X[0] - X[0][1000]) ** 2).sum(1))[:40]
    c = plant("one_in_batch", np.concatenate([X[0][crop[:20]], [[0.5, 0.5, 0.5]], X[0][crop[20:]]]),
              np.concatenate([R[crop[:20]], [3.0], R[crop[20:]]]), sizes=[20, 1, 20])
    assert c[20] == 960
    for P in (1, 64, 960, 1000):
        c = plant(f"crop_P{P}", X[0][crop], R[crop], P=P)
        print(f"crop P = {P}: {int(c.sum())} exposed of {40 * P}")
    out["planted_names"] = np.array(sorted(planted))
    path = os.path.join(OUT, "sasa.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
