"""Writes tests/golden/normalmodes.npz: the named cases of tests/test_normalmodes_fixture.py with what the GPU tests take from a
recording rather than recompute on every run - the coordinates (so that a change of a generator shows), b, the spring count, the
lowest eigenvalues on the complement of R by LAPACK, e_ref (eigvalsh of the matrix against the squared singular values of the spring
incidence matrix) and the deviations LAPACK's own eigenvectors show from orthonormality and from the complement of R. Everything comes
from seeds and from the project's own tests/golden/io_1thf_D.npz.

    python tests/golden/make_normalmodes_golden.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import test_normalmodes_fixture as fx  # noqa: E402


def main():
    out = {}
    for case, (x, kind, cutoff, scale, p, k, nz) in fx.named_cases().items():
        net = fx.Network(x, kind, cutoff, scale, 1.0, p)
        lam = net.eig()[0]
        e_ref = net.e_ref()
        assert not np.any((lam > 1e-14 * net.b) & (lam < 1e-6 * net.b)), case
        assert int((lam <= fx.FLOPPY * net.b).sum()) == nz, case
        out[case + "/x"] = x
        out[case + "/b"] = np.float64(net.b)
        out[case + "/n_springs"] = np.int64(net.n_springs)
        out[case + "/lam"] = lam[:k]
        out[case + "/e_ref"] = np.float64(e_ref)
        out[case + "/dev"] = np.array(net.lapack_dev())
        print(case, "n", net.n, "springs", net.n_springs, "b", net.b, "e_ref / b", e_ref / net.b, "dev", net.lapack_dev(), "lam[:3] / b", lam[:3] / net.b)
    np.savez_compressed(os.path.join(HERE, "normalmodes.npz"), **out)


if __name__ == "__main__":
    main()
