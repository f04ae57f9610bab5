"""The builders of tests/assembly_cases.py on the CPU, before any GPU run: every case reaches the edge its builder claims
(check_claims: pair counts per Schur block from J.observers, entries per pose and factors per landmark from the reference's own
lists), and the joint Gauss-Newton step of gn_reference moves the graph, so that no case can pass vacuously."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assembly_cases as ac                                                    # noqa: E402
from test_joint_reference import joint_reference                               # noqa: E402


@pytest.mark.parametrize("name,make", ac.CASES, ids=[c[0] for c in ac.CASES])
def test_case_reaches_its_edge_and_moves(name, make):
    J, claims = make()
    ref, _ = joint_reference(J, 0)
    ac.check_claims(J, ref, claims)
    dx, _ = ref.step(ref.values)
    assert np.all(np.isfinite(dx)) and np.linalg.norm(dx) > 1e-6


def test_pair_batch_is_the_kernels():
    """PAIR_BATCH is read off the kernel: k_schur_listed_body's pair loop advances by it (eight lanes, three entries each)."""
    src = open(os.path.join(ROOT, "slide_slam_amd", "csrc", "solver_kernels.hip")).read()
    body = src[src.index("void k_schur_listed_body"):src.index("void k_schur_lb(")]
    m = re.search(r"for \(int x0 = q0 \+ sub; x0 < q1; x0 \+= (\d+)\)", body)
    assert m and int(m.group(1)) == ac.PAIR_BATCH
    assert ac.PAIR_BATCH in ac.PAIR_COUNTS and ac.PAIR_BATCH + 1 in ac.PAIR_COUNTS
