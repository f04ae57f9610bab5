"""The builders of tests/assembly_region_cases.py on the CPU, before any GPU run: every case reaches the edge its builder claims
(check_claims: slots, ghost factors, landmarks and padding per robot from J itself), and the joint Gauss-Newton step of gn_reference
moves the graph, so that no case can pass vacuously."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assembly_region_cases as rc                                             # noqa: E402
from test_joint_reference import joint_reference                               # noqa: E402


@pytest.mark.parametrize("name,make", rc.CASES, ids=[c[0] for c in rc.CASES])
def test_case_reaches_its_edge_and_moves(name, make):
    J, claims = make()
    ref, _ = joint_reference(J, 0)
    rc.check_claims(J, ref, claims)
    dx, _ = ref.step(ref.values)
    assert np.all(np.isfinite(dx)) and np.linalg.norm(dx) > 1e-6


def test_builders_are_deterministic():
    for _, make in rc.CASES:
        (a, _), (b, _) = make(), make()
        assert [(c, g, sorted(o)) for c, g, _, o in a.lms] == [(c, g, sorted(o)) for c, g, _, o in b.lms]
        assert all(np.array_equal(x[3], y[3]) and (x[0], x[1], x[2], x[4]) == (y[0], y[1], y[2], y[4]) for x, y in zip(a.relmeas, b.relmeas))


def test_switch_is_the_launchers():
    """The knob the GPU test sets is the one the launchers read, on every call (no function-local static)."""
    src = open(os.path.join(ROOT, "slide_slam_amd", "csrc", "solver_kernels.hip")).read()
    body = src[src.index("AsmMerge asm_merge_env()"):src.index("void launch_phase3_arrow_batched")]
    assert 'getenv("SLIDE_ASM_MERGE")' in body and "static" not in body
    assert src.count("asm_merge_env()") == 3          # (defined once, read by launch_phase3_arrow_batched and launch_arrow_finish_batched)
