"""The step kernels (one block column per launch) and the pair kernel (two per launch) on BORDERED systems with a profile, as the exact
joint passes hand them to the factorisation: a band segment with its active border rows in their own order, the bands'
second level, a leaf of the separator system.  The system is built from a known factor (chol_cases.py): A = L0 L0^T inside a monotone tile
profile, border rows B = W0 L0^T (zero before their first block column), right-hand side b = L0 y0 — so the factorisation must return L0,
W0 and y0.  Here: n_copies of ONE system per launch sequence; different systems side by side in test_gpu_chol_batch.py."""
import pytest

import chol_cases as cc
from chol_cases import CASES

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("method", [0, 2])
@pytest.mark.parametrize("case", sorted(CASES))
def test_bordered_factorisation_returns_the_known_factor(gpu, case, method):
    d = cc.build(CASES[case], case)
    out = gpu.api.debug_chol_bordered(d["S"], d["ld"], d["T"], d["nbr"], prof=d["prof"], bfirst=d["bfirst"], ord=d["ord"], b0=d["b0"], kofs=d["kofs"],
                                      n_copies=CASES[case].get("n_copies", 1), method=method)
    assert gpu.pair_timeouts() == 0
    assert out["copy_diff"] == 0.0, "the copies of one system in a launch sequence differ"
    cc.check_system(d, out)
