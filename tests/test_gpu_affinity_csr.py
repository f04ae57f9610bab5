"""CLIPPER's affinity matrix built as CSR on the device (k_affinity_csr) and the solves that start from it: against the dense path
bit for bit (one shared scoring function), against the oracle, the two-call capacity protocol, and past the dense path's old cap."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import pyoracle as po

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from test_affinity_csr import dense_to_csr  # noqa: E402
from test_oracle_pins import MTRUE, _model_data  # noqa: E402

KW = dict(sigma=0.1, epsilon=0.3)


def _assert_csr_equals_dense(gpu, D1, D2, A, **kw):
    """the device CSR against the CSR of the dense path's M + M.T: pointers, columns and the values' bits"""
    M = gpu.clipper_affinity(D1, D2, A, **kw)
    assert np.array_equal(np.tril(M), np.zeros_like(M))
    want = dense_to_csr(M + M.T)
    got = gpu.clipper_affinity_csr(D1, D2, A, **kw)
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w)
    return got


def _points(rng, n1, n2, dim):
    D1 = rng.uniform(-10, 10, (n1, dim))
    D2 = D1[rng.permutation(n1)[:n2]] + rng.normal(0, 0.02, (n2, dim))
    return D1, D2


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("m", [0, 1, 2, 63, 64, 65, 129, 257])
def test_csr_equals_dense_path_by_size(gpu, m, dim):
    """row counts that are no multiple of the four rows of a workgroup, column counts on either side of a 64-lane chunk; m random
    associations of 40 x 25 points, many sharing an endpoint"""
    rng = np.random.default_rng(100 * dim + m)
    D1, D2 = _points(rng, 40, 25, dim)
    A = np.array([(i, j) for i in range(40) for j in range(25)], np.int32)[rng.permutation(1000)[:m]].reshape(m, 2).copy()
    rowptr, col, val = _assert_csr_equals_dense(gpu, D1, D2, A, **KW)
    assert len(rowptr) == m + 1 and rowptr[0] == 0 and rowptr[-1] == len(col)
    if m >= 63:
        assert 0 < len(col) < m * (m - 1)


@pytest.mark.parametrize("dim", [2, 3])
def test_csr_equals_dense_path_by_kind(gpu, dim):
    rng = np.random.default_rng(7 + dim)
    D1, D2 = _points(rng, 13, 10, dim)
    all_to_all = np.array([(i, j) for i in range(13) for j in range(10)], np.int32)       # m = 130: rows of distinctness zeros
    rowptr, col, _ = _assert_csr_equals_dense(gpu, D1, D2, all_to_all, **KW)
    for k in (0, 57, 129):                                     # no entry between associations that share a point
        c = col[rowptr[k]:rowptr[k + 1]]
        assert not np.any((all_to_all[c, 0] == all_to_all[k, 0]) | (all_to_all[c, 1] == all_to_all[k, 1]))
    n = 97
    D1 = rng.uniform(-10, 10, (n, dim))
    D2 = D1 + rng.normal(0, 0.02, (n, dim))
    ident = np.column_stack([np.arange(n), np.arange(n)]).astype(np.int32)
    r0, c0, _ = _assert_csr_equals_dense(gpu, D1, D2, ident, **KW)
    r1, c1, _ = _assert_csr_equals_dense(gpu, D1, D2, ident, mindist=4.0, **KW)            # mindist > 0 removes the near pairs
    assert 0 < len(c1) < len(c0)
    D2[41] += 1000.0                                           # no distance from 41 matches any more: an empty row (and column)
    r2, c2, _ = _assert_csr_equals_dense(gpu, D1, D2, ident, **KW)
    assert r2[42] == r2[41] and 41 not in c2 and len(c2) > 0


@pytest.mark.parametrize("dim", [1, 4])
def test_csr_equals_dense_path_general_dim(gpu, dim):
    """any other dim takes the kernel that loops over the coordinates (no points in registers)"""
    rng = np.random.default_rng(40 + dim)
    D1, D2 = _points(rng, 40, 25, dim)
    A = np.array([(i, j) for i in range(40) for j in range(25)], np.int32)[rng.permutation(1000)[:129]].copy()
    _, col, _ = _assert_csr_equals_dense(gpu, D1, D2, A, **KW)
    assert 0 < len(col) < 129 * 128


def test_csr_full_matrix(gpu):
    """D2 = D1 with the identity list: every off-diagonal entry is exp(0) = 1.0, nnz = m (m - 1)"""
    m = 130
    D1 = np.random.default_rng(3).uniform(-10, 10, (m, 2))
    ident = np.column_stack([np.arange(m), np.arange(m)]).astype(np.int32)
    rowptr, col, val = _assert_csr_equals_dense(gpu, D1, D1.copy(), ident)
    assert len(col) == m * (m - 1) and np.array_equal(val, np.ones(m * (m - 1)))
    assert np.array_equal(rowptr, (m - 1) * np.arange(m + 1))
    assert np.array_equal(col.reshape(m, m - 1), np.array([[j for j in range(m) if j != i] for i in range(m)]))


def test_csr_golden_case(gpu):
    model, data = _model_data()
    A = np.array([(i, j) for i in range(4) for j in range(3)], np.int32)
    got = gpu.clipper_affinity_csr(model, data, A)
    for g, w in zip(got, dense_to_csr(MTRUE - np.eye(12))):     # the reference's own golden matrix without its identity, exact
        assert g.dtype == w.dtype and np.array_equal(g, w)


def _oracle_params(**kw):
    class OCP(C.Structure):
        _fields_ = [("tol_u", C.c_double), ("tol_F", C.c_double), ("maxiniters", C.c_int), ("maxoliters", C.c_int),
                    ("beta", C.c_double), ("maxlsiters", C.c_int), ("eps", C.c_double), ("affinityeps", C.c_double),
                    ("rescale_u0", C.c_int), ("sigma", C.c_double), ("epsilon", C.c_double), ("mindist", C.c_double)]
    p = OCP()
    po.lib().orc_clipper_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_csr_matches_oracle(gpu):
    """the 30 x 20 case of test_clipper_affinity_matches_golden_and_oracle: the oracle's pattern exactly, its values within that
    test's rtol = 1e-14 (device exp against glibc's)"""
    rng = np.random.default_rng(5)
    D1 = rng.uniform(-10, 10, (30, 2)); D2 = D1[rng.permutation(30)[:20]] + rng.normal(0, 0.03, (20, 2))
    A = np.array([(i, j) for i in range(30) for j in range(20)], np.int32)[::3].copy()
    m = len(A)
    Mo = np.zeros((m, m))
    opp = _oracle_params(**KW)
    po.lib().orc_clipper_affinity(_p(np.ascontiguousarray(D1)), C.c_int(30), _p(np.ascontiguousarray(D2)), C.c_int(20), C.c_int(2),
                                  _p(A.copy()), C.c_int(m), C.byref(opp), _p(Mo))
    wr, wc, wv = dense_to_csr(Mo + Mo.T)
    rowptr, col, val = gpu.clipper_affinity_csr(D1, D2, A, **KW)
    assert len(wc) > 100
    assert np.array_equal(rowptr, wr) and np.array_equal(col, wc)
    assert np.allclose(val, wv, rtol=1e-14, atol=0)


def test_capacity_protocol(gpu):
    rng = np.random.default_rng(21)
    D1, D2 = _points(rng, 40, 25, 2)
    A = np.array([(i, j) for i in range(40) for j in range(25)], np.int32)[::5].copy()
    m = len(A)
    want_r, want_c, want_v = gpu.clipper_affinity_csr(D1, D2, A, **KW)
    true_nnz = len(want_c)
    assert true_nnz > 10
    L = gpu.lib()

    def call(cap):
        rowptr = np.full(m + 1, -7, np.int32)
        col = np.full(true_nnz, -7, np.int32)
        val = np.full(true_nnz, -7.0)
        nnz = C.c_longlong(-1)
        rc = L.slide_clipper_affinity_csr(_p(D1), C.c_int(40), _p(D2), C.c_int(25), C.c_int(2), _p(A), C.c_int(m), C.c_double(0.1),
                                          C.c_double(0.3), C.c_double(0.0), C.c_double(1e-4), _p(rowptr), _p(col), _p(val),
                                          C.c_longlong(cap), C.byref(nnz))
        return rc, nnz.value, rowptr, col, val
    rc, nnz, rowptr, col, val = call(true_nnz - 1)
    assert rc == gpu.api.SLIDE_ERR_CAPACITY and nnz == true_nnz
    assert np.array_equal(rowptr, want_r)                        # still filled
    assert np.all(col == -7) and np.all(val == -7.0)             # untouched
    first = call(true_nnz)
    assert first[0] == 0 and first[1] == true_nnz
    assert np.array_equal(first[2], want_r) and np.array_equal(first[3], want_c) and np.array_equal(first[4], want_v)
    second = call(true_nnz)
    assert second[0] == 0 and all(np.array_equal(a, b) for a, b in zip(first[2:], second[2:]))


def _problem_250():
    """the 250-association problem of test_dense_clique_matches_oracle"""
    rng = np.random.default_rng(11)
    D1 = rng.uniform(-10, 10, (40, 2))
    perm = rng.permutation(40)[:25]
    D2 = D1[perm] + rng.normal(0, 0.02, (25, 2))
    A = np.array([(i, j) for i in range(40) for j in range(25)], np.int32)[::4].copy()
    for k, j in enumerate(perm[:12]):
        A[k] = (j, k)
    return D1, D2, A


def _problem_large(m=1280):
    """the bench's affinity generator: an eighth of the associations true"""
    rng = np.random.default_rng(1)
    D1 = rng.uniform(-100, 100, (m, 2))
    D2 = D1 + rng.normal(0, 0.02, (m, 2))
    A = np.column_stack([np.arange(m), rng.permutation(m)]).astype(np.int32)
    A[: m // 8, 1] = A[: m // 8, 0]
    return D1, D2, A, rng.uniform(0, 1, m)


def test_solve_from_csr_equals_solve_from_dense_one_workgroup(gpu, monkeypatch):
    monkeypatch.delenv("SLIDE_CLIPPER_WGS", raising=False)
    D1, D2, A = _problem_250()
    m = len(A)
    M = gpu.clipper_affinity(D1, D2, A, **KW)
    csr = gpu.clipper_affinity_csr(D1, D2, A, **KW)
    p = gpu.clipper_params(**KW)
    for seed in range(6):
        u0 = np.random.default_rng(seed).uniform(0, 1, m)
        nodes, u, score = gpu.clipper_dense_clique(M, u0, p)
        assert gpu.clipper_last_solve_info()[0] == 1
        n2, u2, s2 = gpu.clipper_dense_clique_csr(*csr, u0, p)
        assert gpu.clipper_last_solve_info()[0] == 1
        assert np.array_equal(nodes, n2) and np.array_equal(u, u2) and score == s2 and len(nodes) >= 3
        assert gpu.api.last_device_ms(gpu.api.MS_CLQ_NNZ) == len(csr[1])


def test_solve_from_csr_equals_solve_from_dense_cooperative(gpu, monkeypatch):
    """m >= 1024: the cooperative multi-workgroup kernel on both sides"""
    monkeypatch.delenv("SLIDE_CLIPPER_WGS", raising=False)
    D1, D2, A, u0 = _problem_large()
    M = gpu.clipper_affinity(D1, D2, A, **KW)
    csr = gpu.clipper_affinity_csr(D1, D2, A, **KW)
    for g, w in zip(csr, dense_to_csr(M + M.T)):
        assert np.array_equal(g, w)
    p = gpu.clipper_params(**KW)
    nodes, u, score = gpu.clipper_dense_clique(M, u0, p)
    assert gpu.clipper_last_solve_info()[0] > 1
    n2, u2, s2 = gpu.clipper_dense_clique_csr(*csr, u0, p)
    assert gpu.clipper_last_solve_info()[0] > 1
    assert np.array_equal(nodes, n2) and np.array_equal(u, u2) and score == s2
    assert len(nodes) >= 0.9 * (len(A) // 8)
    n3, u3, s3 = gpu.clipper_match(D1, D2, A, u0, p)
    assert gpu.clipper_last_solve_info()[0] > 1
    assert np.array_equal(nodes, n3) and np.array_equal(u, u3) and score == s3


def test_clipper_match(gpu, monkeypatch):
    """one call from the associations to the clique = clipper_affinity_csr + clipper_dense_clique_csr bit for bit, and the oracle's
    clique from the same six starts at test_dense_clique_matches_oracle's tolerances"""
    monkeypatch.delenv("SLIDE_CLIPPER_WGS", raising=False)
    D1, D2, A = _problem_250()
    m = len(A)
    p = gpu.clipper_params(**KW)
    op = _oracle_params(**KW)
    csr = gpu.clipper_affinity_csr(D1, D2, A, **KW)
    Mo = np.zeros((m, m))
    po.lib().orc_clipper_affinity(_p(np.ascontiguousarray(D1)), C.c_int(40), _p(np.ascontiguousarray(D2)), C.c_int(25), C.c_int(2),
                                  _p(A.copy()), C.c_int(m), C.byref(op), _p(Mo))
    for seed in range(6):
        u0 = np.random.default_rng(seed).uniform(0, 1, m)
        nodes, u, score = gpu.clipper_match(D1, D2, A, u0, p)
        n2, u2, s2 = gpu.clipper_dense_clique_csr(*csr, u0, p)
        assert np.array_equal(nodes, n2) and np.array_equal(u, u2) and score == s2
        on = np.zeros(m, np.int32); ou = np.zeros(m); osc = C.c_double(0)
        n = po.lib().orc_clipper_solve(_p(Mo), C.c_int(m), _p(u0), C.byref(op), _p(on), _p(ou), C.byref(osc))
        assert sorted(nodes.tolist()) == sorted(on[:n].tolist())
        assert abs(score - osc.value) < 1e-6 * max(1.0, abs(osc.value))
        assert np.abs(u - ou).max() < 1e-6
    nodes, _, _ = gpu.clipper_match(D1, D2, A, None, p)          # library-drawn start weights
    assert len(nodes) >= 3
    nodes, u, score = gpu.clipper_match(D1, D2, A[:0], None, p)  # no association: no clique
    assert len(nodes) == 0 and len(u) == 0 and score == 0.0


# ---- past the dense path's old cap -----------------------------------------------------------------------------------------------
BIG_M = 48000
BIG_NNZ = 108350
PLANTED = [1234, 20000, 40001, 47000]


def big_case():
    rng = np.random.default_rng(48000)
    D1 = rng.uniform(-1000, 1000, (BIG_M, 2))
    D2 = rng.uniform(-1000, 1000, (BIG_M, 2))
    D2[PLANTED] = D1[PLANTED] + np.array([3.5, -2.25])          # four associations that agree on one translation
    A = np.column_stack([np.arange(BIG_M), np.arange(BIG_M)]).astype(np.int32)
    return D1, D2, A


def rows_reference(D1, D2, A, rows, sigma=0.01, epsilon=0.06, mindist=0.0, affinityeps=1e-4):
    """rows of the symmetric diagonal-free matrix, vectorised numpy (clipper.cpp:30-52, euclidean_distance.cpp:13-31): per row
    (columns ascending, values)"""
    P1, P2 = D1[A[:, 0]], D2[A[:, 1]]
    out = []
    for i in rows:
        e1, e2 = P1 - P1[i], P2 - P2[i]
        s1, s2 = np.zeros(len(A)), np.zeros(len(A))
        for k in range(D1.shape[1]):
            s1 += e1[:, k] * e1[:, k]
            s2 += e2[:, k] * e2[:, k]
        l1, l2 = np.sqrt(s1), np.sqrt(s2)
        c = np.abs(l1 - l2)
        with np.errstate(under="ignore"):
            scr = np.where(c < epsilon, np.exp(-0.5 * c * c / (sigma * sigma)), 0.0)
        keep = (scr > affinityeps) & (A[:, 0] != A[i, 0]) & (A[:, 1] != A[i, 1])
        if mindist > 0:
            keep &= ~((l1 < mindist) | (l2 < mindist))
        keep[i] = False
        cols = np.nonzero(keep)[0]
        out.append((cols.astype(np.int32), scr[cols]))
    return out


def test_past_the_old_cap(gpu):
    """m = 48 000 associations (the dense path refused above 46 000; its matrix would be 18.4 GB): two independent uniform sets in
    [-1000, 1000]^2 under the identity list, the reference's default sigma / epsilon / mindist, seed 48000 — 108 350 non-zeros (BIG_NNZ)
    (counted once with rows_reference over all rows on a CPU: 0.005 % of the matrix).  No dense matrix is formed, and the solve
    is not run at this size (its iteration count on such a problem has not been measured)."""
    from scipy.sparse import csr_matrix
    D1, D2, A = big_case()
    rowptr, col, val = gpu.clipper_affinity_csr(D1, D2, A)
    nnz = len(col)
    assert len(rowptr) == BIG_M + 1 and rowptr[0] == 0 and rowptr[-1] == nnz == len(val)
    assert nnz == BIG_NNZ < 4_000_000
    assert gpu.api.last_device_ms(gpu.api.MS_CLQ_NNZ) == nnz and gpu.api.last_device_ms(gpu.api.MS_AFFINITY_CSR) > 0
    rows = [0, BIG_M - 1, PLANTED[0], PLANTED[2]] + sorted(np.random.default_rng(2).choice(BIG_M, 8, replace=False).tolist())
    assert len(set(rows)) == 12
    for i, (wc, wv) in zip(rows, rows_reference(D1, D2, A, rows)):
        gc, gv = col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]
        assert np.array_equal(gc, wc), i
        assert np.allclose(gv, wv, rtol=1e-14, atol=0), i
    for i in (PLANTED[0], PLANTED[2]):                            # the planted rows hold their three partners at ~1.0
        gc, gv = col[rowptr[i]:rowptr[i + 1]], val[rowptr[i]:rowptr[i + 1]]
        for j in PLANTED:
            if j != i:
                assert j in gc and gv[list(gc).index(j)] > 0.999
    S = csr_matrix((val, col, rowptr), shape=(BIG_M, BIG_M))
    inside = np.ones(nnz - 1, bool)                               # columns ascending within every row
    ends = rowptr[1:-1]
    inside[ends[(ends > 0) & (ends < nnz)] - 1] = False
    assert np.all(np.diff(col)[inside] > 0)
    assert (S != S.T).nnz == 0                                    # symmetric, values included
    assert S.diagonal().sum() == 0.0


def test_pipeline_takes_the_sparse_build(gpu):
    """slide_semantic_clipper builds its CSR straight from the associations: SLIDE_MS_AFFINITY_CSR is set by the call and the CSR's
    size is reported"""
    from test_gpu_place import _slidegraph_case
    tm, td, _, _ = _slidegraph_case(0)
    L = gpu.api
    r = gpu.semantic_clipper(tm, td, gpu.clipper_params(sigma=0.05, epsilon=0.2), min_num_pairs=4, matching_threshold=0.1,
                             u0=None)
    assert r["n_putative"] > 0
    assert L.last_device_ms(L.MS_AFFINITY_CSR) > 0
    assert L.last_device_ms(L.MS_CLQ_NNZ) > 0
