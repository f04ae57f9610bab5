"""The one-step reference (tests/gn_reference.py: the full, unreduced whitened Jacobian solved by QR) against the oracle's first
solve, which is one Gauss-Newton step from the initial values (graph.hpp Graph::solve: Schur complement of the landmarks, dense
Cholesky).  Two independent routes to the same step: without this check nobody can trust the reference the GPU step tests use."""
import numpy as np
import pytest

import gn_graphs as gg
from gn_reference import Reference, scaled_error, tolerance
from oracle import pyoracle as po

CASES = [
    ("pose_list_40", lambda G: gg.pose_list_graph(G, 40)),
    ("lm_cyl_25", lambda G: gg.landmark_count_graph(G, 0, 25)),
    ("lm_cube_25", lambda G: gg.landmark_count_graph(G, 1, 25)),
    ("lm_point_65", lambda G: gg.landmark_count_graph(G, 2, 65)),
    ("poses_33", lambda G: gg.pose_count_graph(G, 33)),
    ("full3d", lambda G: gg.geometry_graph(G, "full3d")),
    ("rot3", lambda G: gg.geometry_graph(G, "rot3")),
    ("quat", lambda G: gg.geometry_graph(G, "quat")),
    ("far", lambda G: gg.geometry_graph(G, "far")),
    ("bearing", lambda G: gg.geometry_graph(G, "bearing")),
]


def oracle_values(og, ref):
    """The oracle's estimate in the export's variable layout."""
    out = ref.values.copy()
    for k, key in enumerate(ref.vkey):
        c, idx = int(key) >> 56, int(key) & ((1 << 56) - 1)
        if int(ref.vtype[k]) == po.V_POSE:
            st, v = og.get_pose12("xyzmnopqrstvw".index(chr(c)), idx)
        else:
            st, v = og.get_landmark("lcu".index(chr(c)), idx)
        assert st == 0
        out[k, : len(v)] = v
    return out


def numdiff_floor(ref, dx, H, values=None):
    """How far the rounding noise of the central differences moves the step at `values`: numdiff_delta 1e-6 against 1.00001e-6
    (tools/chart_sensitivity.py's experiment), in the norm of scaled_error.  (A property of the linearisation point: relative to a
    shorter step, later in the descent, it is larger.)"""
    if not np.isin(ref.ftype, (po.F_CUBE, po.F_CYL)).any():
        return 0.0
    dx2, _ = ref.step(values, delta=1.00001e-6)
    return scaled_error(dx2, dx, H)


@pytest.mark.parametrize("chart", [0, 1])
@pytest.mark.parametrize("name,build", CASES, ids=[c[0] for c in CASES])
def test_reference_step_equals_oracle_first_solve(name, build, chart):
    og = po.OracleGraph(po.OrcParams.default(pose_chart=chart))
    build(og)
    ref = Reference(og, chart)
    dx, H = ref.step()
    assert og.solve() == 0
    got = ref.tangent(ref.values, oracle_values(og, ref))
    tol, kappa = tolerance(H, dx, ref.magnitude(ref.values), numdiff_floor(ref, dx, H))
    err = scaled_error(got, dx, H)
    assert np.linalg.norm(dx) > 1e-3                 # (the step really moves the graph)
    assert err <= tol, (err, tol, kappa)
