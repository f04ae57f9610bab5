"""The clique-solver cases of tests/clique_cases.py and their plain numpy reference (tests/clique_reference.py), proven on the CPU
before a GPU sees them: the reference against the C++ oracle on every case; every full-solve case reaches the branch it exists
for; every case is admissible (the reference's float64, permuted and long-double runs take the same decisions, far from every
threshold); the probes show the rows they were built to show.  The tolerances are those of test_gpu_clique_solve.py."""
import ctypes as C
import operator

import numpy as np
import pytest

import clique_cases as cc
import clique_reference as ref
from oracle import pyoracle as po

ALL = cc.names()
OPS = {">=": operator.ge, "==": operator.eq, "<": operator.lt}


class OCP(C.Structure):
    _fields_ = [("tol_u", C.c_double), ("tol_F", C.c_double), ("maxiniters", C.c_int), ("maxoliters", C.c_int),
                ("beta", C.c_double), ("maxlsiters", C.c_int), ("eps", C.c_double), ("affinityeps", C.c_double),
                ("rescale_u0", C.c_int), ("sigma", C.c_double), ("epsilon", C.c_double), ("mindist", C.c_double)]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_case_list_covers_the_sizes_and_rows():
    ns = {cc.case(k)["n"] for k in ALL}
    assert {1, 2, 3, 63, 64, 65, 130, 257, 1023, 1024, 1025, 2049} <= ns
    assert {cc.case(k)["n"] for k in cc.names(kind=("full",))} >= {64, 65, 130, 257, 1023, 1024, 1025}
    for k in ALL:
        c = cc.case(k)
        lengths = np.diff(c["rowptr"])
        for row, length in c["special"]:
            assert lengths[row] == length, (k, row)
        S, _ = ref.csr_to_dense(*cc.csr(c))
        assert np.array_equal(S, S.T) and not S.diagonal().any(), k
    c = cc.case("probe1025-d0.02-u0zeros-C")
    assert (c["u0"] == 0).sum() == (1025 + 2) // 3 and c["params"]["rescale_u0"] == 0
    assert (cc.case("hard130-norescale-u0zeros")["u0"] == 0).sum() == (130 + 2) // 3


@pytest.mark.parametrize("name", ALL)
def test_reference_matches_oracle(name):
    c, r = cc.case(name), cc.reference(name)["run"]
    n = c["n"]
    p = OCP()
    po.lib().orc_clipper_default_params(C.byref(p))
    for k, v in c["params"].items():
        setattr(p, k, v)
    M = cc.dense_upper(c)
    nodes, u, score = np.zeros(n, np.int32), np.zeros(n), C.c_double(0)
    k = po.lib().orc_clipper_solve(_p(M), C.c_int(n), _p(c["u0"]), C.byref(p), _p(nodes), _p(u), C.byref(score))
    tol_u, tol_F = cc.tolerances(name)
    err_u, err_F = np.abs(u - r["u"]), abs(score.value - r["F"])
    print(f"{name}: |u - oracle| {err_u.max():.2e} (tolerance {np.max(tol_u):.2e}), |F - oracle| {err_F:.2e} (tolerance {tol_F:.2e})")
    assert nodes[:k].tolist() == r["nodes"]
    assert np.all(err_u <= tol_u) and err_F <= tol_F


@pytest.mark.parametrize("name", ALL)
def test_case_is_admissible(name):
    R = cc.reference(name)
    assert len(R["runs"]) == (3 if cc.case(name)["n"] < 1023 else 2)
    assert R["same_trace"], [r["trace"]["decisions"][:2] for r in R["runs"]]
    print(f"{name}: smallest decision distance {R['min_dist']:.2e} ({R['min_dist_kind']}), spread of F {R['spread_F']:.2e}, of u {R['spread_u']:.2e}")
    assert R["min_dist"] >= 100.0 * R["spread_F"]


@pytest.mark.parametrize("name", cc.names(kind=("full",)))
def test_full_solve_reaches_its_branch(name):
    q = cc.quantities(name)
    print(name, {k: q[k] for k in ("evals", "backtracks", "deepest", "maxls", "maxin", "maxol", "d_updates", "d_grows", "outer", "F", "n_nodes")})
    for key, op, value in cc.case(name)["must"]:
        assert OPS[op](q[key], value), (key, op, value, q[key])


@pytest.mark.parametrize("name", cc.names(kind=("M-probe", "C-probe")))
def test_probe_shows_its_rows(name):
    c, R = cc.case(name), cc.reference(name)
    r = R["run"]
    assert r["trace"]["evals"] == 2 and len(r["trace"]["outer"]) == 1 and r["trace"]["outer"][0][0] == 1
    u1 = r["u"]
    if c["kind"] == "M-probe":
        assert r["d"] == 0.0 and r["trace"]["active"] == (0, 0) and r["clamped_last"] == 0
        if c["params"].get("rescale_u0", 1):
            assert np.all(u1 > 0)
    else:
        if c["n"] >= 63:
            assert r["d"] > 0.0
            assert (u1 > 0).mean() >= 0.4, (u1 > 0).mean()
        for row, length in c["special"]:
            if length >= 63:
                assert u1[row] > 0, (row, length)
    # the bound the GPU test uses holds between the reference's own runs, and is tight enough to see one missing term of a row
    eu, eF = ref.probe_error_bound(cc.csr(c), c["u0"], c["params"])
    for other in R["runs"][1:]:
        assert np.all(np.abs(other["u"] - u1) <= 2 * eu) and abs(other["F"] - r["F"]) <= 2 * eF
    pos = u1 > 0
    print(f"{name}: bound on u1 at most {eu.max():.2e} (relative to u1 {np.max(eu[pos] / u1[pos]):.2e}), on F {eF:.2e}; unclamped {(u1 > 0).mean():.2f}")
    assert eu.max() < 1e-9 and eF < 1e-9 * max(1.0, abs(r["F"]))


def test_rounding_follows_the_heap_scan():
    """k_largest: a later entry enters only if strictly larger than the heap's top, the top being the smallest (value, index) pair —
    of two equal values the smaller index leaves first; the order is largest (value, index) first."""
    assert ref.k_largest([0.5, 0.7, 0.5, 0.7, 0.1], 3) == [3, 1, 2]          # 0.7 at 3 pushes out (0.5, 0), not (0.5, 2)
    assert ref.k_largest([0.5, 0.5, 0.5], 2) == [1, 0]                       # an equal value does not enter
    assert ref.k_largest([0.5, 0.7], 0) == [] and ref.k_largest([0.5, 0.7], -3) == []
    assert ref.k_largest([0.2, 0.9], 5) == [1, 0]
    assert [ref.round_half_away(x) for x in (0.5, 1.5, 2.5, -0.5, -22.9, 0.49)] == [1, 2, 3, -1, -23, 0]
