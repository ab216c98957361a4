"""Frame-to-model tracking without a GPU: the numpy restatement (tests/_point_to_plane_ref.py) against the analytic renderer's
known motion, and the C ABI's declarations of the point-to-plane entries."""
import os
import re

import numpy as np
import pytest

import _point_to_plane_ref as P2P
from _point_to_plane_ref import FULL, K_FULL, K_SMALL, MEDIUM, SMALL, pair

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name, motion, K, hw, holes", [
    ("small", SMALL, K_SMALL, (120, 160), False),
    ("medium", MEDIUM, K_SMALL, (120, 160), False),
    ("medium-holes", MEDIUM, K_SMALL, (120, 160), True),
    ("full-size", FULL, K_FULL, (480, 640), False),
])
def test_restatement_recovers_the_rendered_motion(name, motion, K, hw, holes):
    """6 / 3 / 1 point-to-plane iterations against analytic truth.  Bounds: the values measured for this statement on the CPU
    (worst case 2.7e-6 m, 1.3e-4) with about 3x / 2x room for an equivalent summation order."""
    pose_s, ds, dt = pair(motion, K, *hw, holes=holes)
    trace = []
    T = P2P.point_to_plane(ds, dt, K, 3.0, trace=trace)
    et, er = np.abs(T[:3, 3] - pose_s[:3, 3]).max(), np.abs(T[:3, :3] - pose_s[:3, :3]).max()
    print(f"{name}: translation error {et:.2e} m, rotation error {er:.2e}, inliers {trace[-1][4]} of {hw[0] * hw[1]}")
    assert len(trace) == 10 and [t[0] for t in trace] == [2] * 6 + [1] * 3 + [0]
    assert et <= 1e-5 and er <= 3e-4


def test_normals_are_invalid_where_the_statement_says():
    d = np.full((6, 8), 0.5)
    d[2, 3] = np.nan
    n = P2P.normal_map(P2P.vertex_map(d, (10.0, 10.0, 4.0, 3.0)))
    bad = np.isnan(n).any(-1)
    want = np.zeros((6, 8), bool)
    want[-1, :], want[:, -1] = True, True
    want[2, 3] = want[2, 2] = want[1, 3] = True          # the pixel itself, its left neighbour (u + 1) and the one above it (v + 1)
    assert np.array_equal(bad, want)
    assert np.allclose(n[~bad], (0.0, 0.0, 1.0))         # a fronto-parallel plane: the normal is the optical axis


def test_point_to_plane_entries_are_declared():
    """the header and _lib.EXPORTS both carry the new entries"""
    from bodyslam_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "bodyslam_hip.h")).read()
    declared = set(re.findall(r"\b(bs_[a-z0-9_]+)\s*\(", hdr))
    for name in ("bs_odo_p2p_step", "bs_odo_p2p_accumulate", "bs_odo_p2p_target", "bs_odo_p2p_prepare"):
        assert name in declared and name in _lib.EXPORTS, name
