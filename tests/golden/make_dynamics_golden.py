#!/usr/bin/env python3
"""Generate the dynamics golden (tests/golden/dynamics.npz). Our own generator: no reference code is involved, everything runs on the CPU
in NumPy. The inputs are not stored: the planted-spectrum, flat, cancellation and rank-deficient cases are rebuilt from their seeds and
the md29 case refers to the 29 frames of frames_md_1JTG_uL.npz by index (sel = arange(0, 2030, 7)); the recipes and the float64
yardstick live in tests/test_dynamics_fixture.py (PCA_CASES, case_inputs, Yardstick), which this script imports.

Recorded per case <name>:
  <name>_lam        the first min(33, 3n) eigenvalues of the float64 covariance (np.linalg.eigh), descending
  <name>_e_ref_eig  max |eigvalsh(C) - svd(scale D)^2 / (F - ddof)|: two independent float64 routes to the eigenvalues
  <name>_e_ref_sum  max |C in float64 - C summed in np.longdouble|
  <name>_orth_dev   max |V^T V - I| of eigh's own eigenvectors
  <name>_total      tr C
  <name>_min_gap    the smallest gap among the significant ones (> 1e-11 lam_0) of the first k + 1 eigenvalues
  <name>_rmsf       the float64 RMSF (md29_sel and one_atom_17x21 only)
Asserted here: in every case that must converge the significant eigenvalues among the first k + 1 are distinct, more than
10 (1e-9 lam_0 + 4 e_ref) apart, so Weyl's bound matches them index by index; and no eigenvalue among the first k lies within
1e-14 .. 1e-10 of lam_0, so the rank does not hang on rounding.

Usage:  python tests/golden/make_dynamics_golden.py
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from test_dynamics_fixture import PCA_CASES, yard  # noqa: E402


def main():
    out = {}
    for case in sorted(PCA_CASES):
        (xyz, sel, scale, ddof, k), y = yard(case)
        lam = y.eig()[0]
        e_eig, e_sum = y.e_ref_eig(), y.e_ref_sum()
        head = lam[:k + 1]
        sig = head[head > 1e-11 * lam[0]] if lam[0] > 0 else head[:0]
        gap = float((-np.diff(sig)).min()) if sig.size > 1 else 0.0
        if PCA_CASES[case]["converge"] and sig.size > 1:
            assert gap > 10.0 * (1e-9 * lam[0] + 4.0 * e_eig), (case, gap, lam[0], e_eig)
        if PCA_CASES[case]["converge"] and lam[0] > 0:
            assert not np.any((lam[:k] > 1e-14 * lam[0]) & (lam[:k] < 1e-10 * lam[0])), case
        if "rank" in PCA_CASES[case]:
            assert int((lam[:k] > 1e-12 * lam[0]).sum()) == PCA_CASES[case]["rank"] if lam[0] > 0 else PCA_CASES[case]["rank"] == 0
        out[case + "_lam"] = lam[:min(33, y.m)]
        out[case + "_e_ref_eig"] = np.float64(e_eig)
        out[case + "_e_ref_sum"] = np.float64(e_sum)
        out[case + "_orth_dev"] = np.float64(y.eigh_orth_dev())
        out[case + "_total"] = np.float64(np.trace(y.C))
        out[case + "_min_gap"] = np.float64(gap)
        if case in ("md29_sel", "one_atom_17x21"):
            out[case + "_rmsf"] = y.rmsf
        print(f"{case}: F={y.F} m={y.m} lam0={lam[0]:.3e} e_ref_eig={e_eig:.1e} e_ref_sum={e_sum:.1e} orth={y.eigh_orth_dev():.1e} gap/lam0={gap / max(lam[0], 1e-300):.1e}")
    np.savez_compressed(os.path.join(OUT, "dynamics.npz"), **out)
    print(os.path.getsize(os.path.join(OUT, "dynamics.npz")), "bytes")


if __name__ == "__main__":
    main()
