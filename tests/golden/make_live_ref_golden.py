#!/usr/bin/env python3
"""Records live_ref_golden.npz: the compiled reference Matrix class's answers (oracle/_ref, `make -C oracle ref` where the
reference checkout exists) to the cases of tests/test_oracle_solves.py's test_live_reference_* tests, so that those tests
compare against the reference on a machine without it.

    python tests/golden/make_live_ref_golden.py

nm_pts  -- the 2 000-point map the normals are taken on (float32 xy; the test checks its own input against it)
nm_n    -- computeNormal's U column of the K = 10 neighbour set of every seventh point (ref_normal2)
p2p_R   -- V*U^T of 2 000 cross-covariances, then of the all-zero one (ref_p2p_rotation)
The fixture holds data only: inputs and expected outputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import oracle_lib as O  # noqa: E402
from test_oracle_solves import live_matrix_cases, live_normal_cases  # noqa: E402


def main():
    assert O.ref_available(), "build oracle/_ref first: make -C oracle ref"
    _, pts, cases = live_normal_cases()
    nm_n = np.array([O.ref_normal2(pts[nb]) for _, nb in cases])
    p2p_R = np.array([O.ref_p2p_rotation(H) for H in live_matrix_cases()])
    out = os.path.join(HERE, "live_ref_golden.npz")
    np.savez_compressed(out, nm_pts=pts, nm_n=nm_n, p2p_R=p2p_R)
    print("wrote %s: %d normals, %d rotations" % (out, len(nm_n), len(p2p_R)))


if __name__ == "__main__":
    main()
