#!/usr/bin/env python3
"""Record tests/golden/edge_item_pipeline_parent.npz: the logits of every case of tests/test_edge_item_pipeline.py (which holds the
recipes: model, seeds, atom counts) as the library in the tree computes them on the GPU. Our own generator: no reference code is
involved. The committed file was recorded from a build of the commit BEFORE the item pipeline of the node-wave kernels, so that the
test pins the pipeline to the earlier bits; re-record only from such a build.

Stored: the rendezvous-mode logits (pesto_debug_edge_mode 1). Asserted here: they are finite, a second run gives the same bits, and
modes 0 (per launch) and 2 (node waves) agree with them bit for bit.

Usage (on a machine with an MI355X):  python tests/golden/make_edge_item_pipeline_golden.py [output.npz]
"""
import os
import sys

import numpy as np

OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
sys.path.insert(0, os.path.dirname(os.path.dirname(OUT)))

from test_edge_item_pipeline import GOLDEN_NAME, MODES, case_names, run_case  # noqa: E402


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(OUT, GOLDEN_NAME + ".npz")
    out = {}
    for name in case_names():
        z = np.asarray(run_case(name, 1))
        assert np.isfinite(z).all(), name
        assert np.array_equal(z, run_case(name, 1)), name
        for mode in MODES:
            assert np.array_equal(z, run_case(name, mode)), (name, mode)
        out[name] = z
        print(f"{name}: z{z.shape} |z|max={np.abs(z).max():.3f}")
    np.savez_compressed(path, **out)
    print(os.path.getsize(path), "bytes ->", path)


if __name__ == "__main__":
    main()
