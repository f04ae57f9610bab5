"""The CLIPPER clique solver on the device (clq_solve_body in clipper_kernels.hip, behind k_clq_solve, k_clq_solve_b and
k_clq_solve_coop) branch by branch and row by row, against the plain numpy reference of tests/clique_reference.py on the cases of
tests/clique_cases.py (test_clique_reference.py proves cases and reference on the CPU first).

Every call goes through clipper_dense_clique_csr, so a test hands over exactly the CSR it means; clipper_last_solve_info() gives the
workgroup count and the gradient-evaluation count.  On one workgroup every case must take the reference's path — the same number of
gradient evaluations, exactly — and return its nodes in its order and its u and F within a DERIVED tolerance.  The cooperative kernel
(any workgroup count, more waves than rows included) and the batch kernel must then equal the one-workgroup solve bit for bit, and
the dense entry point (k_clq_csr in front) the CSR entry point.

Tolerance of the PROBE cases (two gradient evaluations, one projected step; every row's sum shows in the result): twice the forward
error bound clique_reference.probe_error_bound derives — the device and the reference each lie within the bound of the exact result.
The bound is first order in e = 2^-53 and holds for any order of summation (|fl(sum) - sum| <= (k - 1) e sum|terms| for k terms;
one e per product, quotient, root), so it covers the device's 64-lane xor tree and its 16 partial sums as it covers numpy:
  w = M u0 + u0            L_i + 1 non-negative terms per row                    relative (L_i + 2) e
  u = w / |w|              n squares, a root, a quotient                         relative r_i = rel(w_i) + max rel(w) + (n/2 + 2) e
  sum u, C u, M u          n, L_i, L_i non-negative terms                        relative max r + (n, L_i, L_i + 1) e
  Cbu = sum u - C u - u    cancels: absolute, the operands' errors + 2 e (their magnitudes)
  d = mean (M u + u) / Cbu over the active set      relative per quotient rel(numerator) + abs(Cbu_i) / Cbu_i + 2 e, the mean (cnt + 1) e
  g = (1 + d) u - d sum u + M u + d C u             absolute: |u_i - sum u + (C u)_i| err(d) + each term's error + 4 e (sum of magnitudes)
  x = max(u + g, 0), u1 = x / |x|                   max is 1-Lipschitz; |x| from n squares: (n/2 + 2) e
  F = u1 . g(u1)           n terms                  sum (u1_i err(g_i) + err(u1_i) |g_i|) + (n + 1) e sum |u1_i g_i|
In the M-probe no constraint is active, d = 0 exactly and every sum is of non-negative terms; the bound on u1 is then a few hundred
e relative.  Tolerance of the FULL solves: measured, not assumed — 1000 times the largest difference in u (in F) between the
reference's own float64, permuted and long-double runs, floored at 1e-12: the margin of 1000 for the device's other reduction
trees over a few hundred contractive iterations.  Every test prints spread, tolerance and achieved error."""
import os

import numpy as np
import pytest

import clique_cases as cc
import clique_reference as ref

pytestmark = pytest.mark.gpu

_ONE = {}


def _solve(gpu, c, wgs):
    """clipper_dense_clique_csr under SLIDE_CLIPPER_WGS = wgs (None: unset) -> (nodes, u, F, workgroups, evaluations)."""
    p = gpu.clipper_params(**c["params"])
    old = os.environ.pop("SLIDE_CLIPPER_WGS", None)
    try:
        if wgs is not None:
            os.environ["SLIDE_CLIPPER_WGS"] = str(wgs)
        nodes, u, score = gpu.clipper_dense_clique_csr(c["rowptr"], c["col"], c["val"], c["u0"], p)
        w, e = gpu.clipper_last_solve_info()
    finally:
        os.environ.pop("SLIDE_CLIPPER_WGS", None)
        if old is not None:
            os.environ["SLIDE_CLIPPER_WGS"] = old
    return nodes, u, score, w, e


def _one_workgroup(gpu, name):
    if name not in _ONE:
        _ONE[name] = _solve(gpu, cc.case(name), 1)
    return _ONE[name]


@pytest.mark.parametrize("name", cc.names())
def test_one_workgroup_follows_the_reference(gpu, name):
    c, R = cc.case(name), cc.reference(name)
    r = R["run"]
    nodes, u, F, w, evals = _one_workgroup(gpu, name)
    tol_u, tol_F = cc.tolerances(name)
    err_u, err_F = np.abs(u - r["u"]), abs(F - r["F"])
    tol_u = np.broadcast_to(tol_u, u.shape)
    exact = tol_u == 0                                   # an entry the bound leaves no room: u0_i = 0 in a row without entries
    ratio = max(float(np.max(err_u[~exact] / tol_u[~exact], initial=0.0)), err_F / tol_F)
    print(f"{name} [{c['edge']}]: evaluations {int(evals)} (reference {r['trace']['evals']}); reference spread u {R['spread_u']:.2e} F {R['spread_F']:.2e}; "
          f"tolerance u {np.max(tol_u):.2e} F {tol_F:.2e}; error u {err_u.max():.2e} F {err_F:.2e}; error / tolerance {ratio:.3g}")
    assert w == 1
    assert evals == r["trace"]["evals"]
    assert nodes.tolist() == r["nodes"]
    assert np.all(err_u <= tol_u), (int(np.argmax(err_u - tol_u)), err_u.max())
    assert err_F <= tol_F


def _coop_params():
    out = []
    for name in cc.names():
        n = cc.case(name)["n"]
        if n in (65, 130, 257):          # 130: the deep line searches, up to 2131 barriers
            out += [(name, w) for w in (None, 2, 37, 256)]
        elif n in (1023, 1024, 1025, 2049):
            out += [(name, w) for w in (None, 37)]
    return out


@pytest.mark.parametrize("name,wgs", _coop_params())
def test_workgroup_count_changes_no_bit(gpu, name, wgs):
    """The cooperative kernel at 2, 37 and 256 workgroups (256: far more waves than rows, whole workgroups own no row and still
    reach every barrier) and at the default count (1 below n = 1024) against the one-workgroup solve: n = 65, 130 and 257; from
    n = 1023 on the default count and 37."""
    c = cc.case(name)
    n1, u1, F1, w1, e1 = _one_workgroup(gpu, name)
    nodes, u, F, w, evals = _solve(gpu, c, wgs)
    want = wgs if wgs is not None else (1 if c["n"] < 1024 else min(128, (c["n"] + 63) // 64))
    assert w1 == 1 and w == want, (w, want)
    assert evals == e1
    assert F == F1 and np.array_equal(u, u1) and np.array_equal(nodes, n1), (evals, e1, F - F1, np.abs(u - u1).max())


BATCH = [None, "probe-n1-C", "probe-n2-edge-C", "probe-n64-C", "probe-n65-C", "hard130", "rows257", "complete64", "isolated65", "noise1025"]


def test_batch_equals_single_solves(gpu):
    """One clipper_dense_clique_batch call (k_clq_solve_b, a workgroup per job, default parameters) over problems of very different
    size and length, an empty one first: every job bit-identical to its own one-workgroup solve of the same CSR."""
    cases = [None if k is None else dict(cc.case(k), params={}) for k in BATCH]
    Ms = [np.zeros((0, 0)) if c is None else cc.dense_upper(c) for c in cases]
    res = gpu.clipper_dense_clique_batch(Ms, [None if c is None else c["u0"] for c in cases], gpu.clipper_params())
    assert len(res) == len(BATCH) and len(res[0][0]) == 0 and len(res[0][1]) == 0
    for c, (bn, bu, bF) in zip(cases[1:], res[1:]):
        nodes, u, F, w, evals = _solve(gpu, c, 1)
        assert w == 1 and evals >= 2
        assert bF == F and np.array_equal(bu, u) and np.array_equal(bn, nodes), (c["name"], bF - F)


def test_batch_equals_single_dense_calls(gpu):
    """The job set-up of clipper_dense_clique_batch against the single call's, from the dense matrices both entry points take:
    n = 0, 1, 3, 64, 65 and 130 in ONE call, the n = 65 job with a caller's u0 and every other job with the default start.  nodes, u
    and score of every job equal clipper_dense_clique's bit for bit ("Results equal n_jobs single calls", include/slide_gpu.h)."""
    mats = {0: (np.zeros((0, 0)), None), 1: cc.noise(1, 0.5, 0.2, 1.0, 411)[:2], 3: cc.chunk_boundary_matrix(3, 413),
            64: cc.planted(64, 8, 0.1, 464)[:2], 65: cc.chunk_boundary_matrix(65, 465), 130: cc.planted(130, 12, 0.08, 530)[:2]}
    ns = [0, 1, 3, 64, 65, 130]
    Ms = [np.ascontiguousarray(np.triu(mats[n][0], 1)) for n in ns]
    u0s = [mats[n][1] if n == 65 else None for n in ns]
    assert np.count_nonzero(Ms[2]) and np.count_nonzero(Ms[3]) and np.count_nonzero(Ms[5])
    res = gpu.clipper_dense_clique_batch(Ms, u0s, gpu.clipper_params())
    assert len(res) == len(ns)
    for n, M, u0, (bn, bu, bF) in zip(ns, Ms, u0s, res):
        nodes, u, F = gpu.clipper_dense_clique(M, u0, gpu.clipper_params())
        print(f"n = {n}: {len(nodes)} nodes, F = {F!r} (batch {bF!r})")
        assert len(bu) == n
        assert bF == F and np.array_equal(bu, u) and np.array_equal(bn, nodes), (n, bF - F)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129, 257])
def test_dense_entry_equals_csr_entry(gpu, n):
    """k_clq_csr (one wave per row, the columns in chunks of 64, ballot ranks) with entries on both sides of every chunk boundary:
    clipper_dense_clique of the upper-filled matrix = clipper_dense_clique_csr of the CSR numpy builds, bit for bit."""
    S, u0 = cc.chunk_boundary_matrix(n, 300 + n)
    rowptr, col, val = ref.dense_to_csr(S)
    if n > 64:
        assert S[0, 63] != 0 and S[0, 64] != 0 and S[n - 1, 63] != 0 and S[1, n - 1] != 0
    c = dict(rowptr=rowptr, col=col, val=val, u0=u0, params={})
    n2, u2, F2, w2, e2 = _solve(gpu, c, 1)
    old = os.environ.pop("SLIDE_CLIPPER_WGS", None)
    try:
        os.environ["SLIDE_CLIPPER_WGS"] = "1"
        nodes, u, F = gpu.clipper_dense_clique(np.ascontiguousarray(np.triu(S, 1)), u0, gpu.clipper_params())
        w, e = gpu.clipper_last_solve_info()
    finally:
        os.environ.pop("SLIDE_CLIPPER_WGS", None)
        if old is not None:
            os.environ["SLIDE_CLIPPER_WGS"] = old
    assert w == w2 == 1 and e == e2
    assert F == F2 and np.array_equal(u, u2) and np.array_equal(nodes, n2)
