"""The assembly kernels of an exact joint pass at their edges — k_schur_lb (pair entries loaded three per lane before the records, record
columns two at a time, adjacency words straight from the bitmap), k_lin_lf_b (the 32-lane region over each graph's list of cubes and
cylinders) and k_pose_b (1, 31 .. 33, 63 .. 65 and 130 entries per pose): every case of tests/assembly_cases.py, two exact
joint passes each (the second starts from the first's result) against the independent joint Gauss-Newton step exactly as
test_gpu_joint_step.py takes it (gn_reference by QR, its own tolerance).  The evidence callback asserts the claimed counts on the host:
entries per pose and factors per landmark from ref.list_lengths(), pairs per Schur block from J.observers."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import assembly_cases as ac                                                    # noqa: E402
from test_gpu_joint_step import run_case                                       # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("chart", [0, 1], ids=["chart0", "expmap"])
@pytest.mark.parametrize("name,make", ac.CASES, ids=[c[0] for c in ac.CASES])
def test_assembly_edges(gpu, monkeypatch, name, make, chart):
    monkeypatch.delenv("SLIDE_SCHUR_WALK", raising=False)
    J, claims = make()

    def ev(r):
        ac.check_claims(J, r.ref, claims)
        assert r.info["n_slots"] > 0
    _, ratio = run_case(gpu, J, chart, evidence=ev)
    print(f"[assembly-edges] {name}: worst scaled_error / tolerance {ratio:.3e}")
