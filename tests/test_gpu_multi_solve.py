"""The many-column substitutions (k_sub_fwd, k_sub_bwd through launch_multi_solve / launch_multi_fwd with its short walk k0), the gram
product (k_gram) and the single-pose walk (k_cov_fwd, k_cov_gram) on caller-built factors (cov_cases.py), through slide_debug_multi_solve,
slide_debug_gram and slide_debug_pose_covariance.

The information gain, the closure / observation / predicted-pose / joint-compatibility / landmark-pair gates all stand on these launches
and promise that a candidate's bits do not depend on what else is in the launch; launch_multi_fwd promises that rows from k0 * 64 on
"come out with the bits of the walk from column 0".  Both promises are checked here at the kernel: a column alone against the same
column at every position of a 33-column launch (chunk edges at 15, 16, 17), the short walk against the full one for k0 at 1, T / 2 and
T - 1.  Values are held to bound (c) of cov_cases.py against long-double solves (k_gram to the a-priori bound (a) with K = nrows);
columns at or beyond nrhs, rows above the short walk, the gram's guard row and Y above the pose's tile must keep their bits.

Worst |err| / bound observed on an MI355X (profiles/cov_kernels_bounds.txt): (c) X 0.134 (stairs, 33 dense columns), (c) W 0.125, k_gram (a)
0.196 (one row; 0.02 - 0.07 from 63 rows on), cov36 (c) 0.160 (row0 = 0).  Every bit-for-bit condition held; no kernel needed a change."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import cov_cases as cc                                                         # noqa: E402
from cov_cases import LD, NB                                                   # noqa: E402

pytestmark = pytest.mark.gpu
SOLVE_CASES = ["band3", "stairs", "dense5"]
NRHS = [1, 15, 16, 17, 33]
ALLOC = cc.NCOL + 2                                                            # two columns behind the widest launch


def _report(what, **ratios):
    print(f"[multi-solve] {what}: " + "  ".join(f"{k} {v:.3e}" for k, v in ratios.items()))


def _factor(name):
    m = cc.profile_model(name)
    return m, cc.factor_layout(m, cc.lds_of(m["Tc"], True))


def _buffers(B, n):
    """B in the first rows of an ALLOC-column buffer whose other columns hold OUT_NAN, and an X buffer of OUT_NAN."""
    Bb = np.full((ALLOC, n), cc.OUT_NAN)
    Bb[:B.shape[0]] = B
    return Bb, np.full((ALLOC, n), cc.OUT_NAN)


def _err_ratio(got, ref, tol):
    e = np.abs(got.astype(LD) - ref).astype(np.float64)
    return float(e.max() / tol) if np.all(np.isfinite(e)) else np.inf


@pytest.mark.parametrize("kind", ["dense", "unit"])
@pytest.mark.parametrize("nrhs", NRHS)
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_solve_and_forward(gpu, name, nrhs, kind):
    m, f = _factor(name)
    n = m["Tc"] * NB
    r = cc.solve_reference(name, kind)
    Bb, Xb = _buffers(r["B"], n)
    Bb[nrhs:] = cc.OUT_NAN                                                      # (the columns behind nrhs are nobody's business)
    _, X = gpu.api.debug_multi_solve(f, Bb, Xb, nrhs, mode=0)
    B1, W = gpu.api.debug_multi_solve(f, Bb, Xb, nrhs, mode=1)
    for got in (X, W, B1):
        assert cc.same_bits(got[nrhs:], Xb[nrhs:]), "a column at or beyond nrhs was written"
    assert not np.isnan(X[:nrhs]).any() and not np.isnan(W[:nrhs]).any(), "a NaN: a read outside the contract, or rows left unwritten"
    rx, rw = _err_ratio(X[:nrhs], r["X"][:nrhs], r["tol_X"]), _err_ratio(W[:nrhs], r["W"][:nrhs], r["tol_W"])
    _report(f"{name} nrhs {nrhs} {kind}", c_X=rx, c_W=rw)
    assert rx <= 1 and rw <= 1


@pytest.mark.parametrize("kind", ["dense", "unit"])
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_column_alone_or_in_a_chunk(gpu, name, kind):
    """Column c has the same bits alone (nrhs = 1) as at every position inside nrhs = 33: c is rotated through positions that cover every
    lane of a chunk and all three chunks."""
    m, f = _factor(name)
    n = m["Tc"] * NB
    B = cc.solve_reference(name, kind)["B"]
    c = 5
    Bb, Xb = _buffers(B[c:c + 1], n)
    _, x1 = gpu.api.debug_multi_solve(f, Bb, Xb, 1, mode=0)
    _, w1 = gpu.api.debug_multi_solve(f, Bb, Xb, 1, mode=1)
    for shift in (0, 1, 11, 16, 27):                                          # column c sits at (c + shift) % 33: 5, 6, 16, 21, 32
        Bs = np.roll(B, shift, axis=0)
        Bb, Xb = _buffers(Bs, n)
        _, X = gpu.api.debug_multi_solve(f, Bb, Xb, cc.NCOL, mode=0)
        _, W = gpu.api.debug_multi_solve(f, Bb, Xb, cc.NCOL, mode=1)
        pos = (c + shift) % cc.NCOL
        assert cc.same_bits(X[pos], x1[0]), ("solve", pos)
        assert cc.same_bits(W[pos], w1[0]), ("forward", pos)
    # and every position of one launch against that position's column launched alone
    Bb, Xb = _buffers(B, n)
    _, X = gpu.api.debug_multi_solve(f, Bb, Xb, cc.NCOL, mode=0)
    _, W = gpu.api.debug_multi_solve(f, Bb, Xb, cc.NCOL, mode=1)
    for pos in range(cc.NCOL):
        b1, x0 = _buffers(B[pos:pos + 1], n)
        assert cc.same_bits(gpu.api.debug_multi_solve(f, b1, x0, 1, mode=0)[1][0], X[pos]), ("solve", pos)
        assert cc.same_bits(gpu.api.debug_multi_solve(f, b1, x0, 1, mode=1)[1][0], W[pos]), ("forward", pos)


@pytest.mark.parametrize("kind", ["dense", "unit"])
@pytest.mark.parametrize("name", SOLVE_CASES)
def test_short_walk(gpu, name, kind):
    """k0 in {1, T / 2, T - 1}: B zero above row 64 k0, W zeroed there by the caller.  Rows from 64 k0 on have the bits of the walk from
    column 0; the rows above are untouched."""
    m, f = _factor(name)
    T, n = m["Tc"], m["Tc"] * NB
    for k0 in sorted({1, T // 2, T - 1}):
        B = cc.rhs(m, kind, k0)
        assert not B[:, :NB * k0].any()
        Bb, Xb = _buffers(B[:17], n)
        Xb[:17, :NB * k0] = 0.0
        _, W0 = gpu.api.debug_multi_solve(f, Bb, Xb, 17, mode=1, k0=0)
        Bk, Wk = gpu.api.debug_multi_solve(f, Bb, Xb, 17, mode=1, k0=k0)
        assert cc.same_bits(Wk[:17, NB * k0:], W0[:17, NB * k0:]), ("rows from 64 k0 on differ from the walk from column 0", k0)
        assert cc.same_bits(Wk[:, :NB * k0], Xb[:, :NB * k0]) and cc.same_bits(Bk[:, :NB * k0], Bb[:, :NB * k0]), ("rows above the short walk were written", k0)
        assert cc.same_bits(Wk[17:], Xb[17:])
        assert not np.isnan(Wk[:17]).any()


# ---- k_gram ---------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("nrows", cc.GRAM_NROWS)
@pytest.mark.parametrize("ncol", cc.GRAM_NCOL)
def test_gram(gpu, ncol, nrows):
    worst = 0.0
    for lst in cc.GRAM_LISTS:
        X, rows, M0, ref, bound = cc.gram_case(ncol, nrows, lst)
        M = gpu.api.debug_gram(X, rows, nrows, M0)
        assert cc.same_bits(M[ncol], M0[ncol]), "the guard row behind M was written"
        G = M[:ncol]
        assert not np.isnan(G).any(), "a NaN: a row outside the list was read"
        assert cc.same_bits(G, G.T), "M is not symmetric bit for bit"
        err = np.abs(G.astype(LD) - ref).astype(np.float64)
        worst = max(worst, float((err / bound).max()))
    X, _, M0, _, _ = cc.gram_case(ncol, nrows, "null")                          # the identity list on the null case's own X
    a = gpu.api.debug_gram(X, None, nrows, M0)
    b = gpu.api.debug_gram(X, np.arange(nrows, dtype=np.int32), nrows, M0)
    assert cc.same_bits(a, b), "the identity list and NULL differ in bits"
    _report(f"gram ncol {ncol} nrows {nrows}", a=worst)
    assert worst <= 1


# ---- the single-pose walk ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row0", [0, 60, 762, 704], ids=["first", "straddles_tiles_0_1", "last_pose", "first_row_of_last_tile"])
def test_pose_covariance(gpu, row0):
    """band3 with S zero outside the profile (k_cov_fwd walks the dense column).  row0 = 60: pose 10 holds rows 60 .. 65."""
    m = cc.profile_model("band3")
    n = m["Tc"] * NB
    assert n == 768 and 6 * ((n - 6) // 6) == 762
    f = cc.factor_layout(m, cc.lds_of(m["Tc"], True), zero_outside=True)
    cov, Y = gpu.api.debug_pose_covariance(f, row0)
    ref, tol, _ = cc.pose_cov_reference("band3", row0)
    assert not np.isnan(cov).any() and not np.isnan(Y).any()
    k = row0 // NB
    assert cc.same_bits(Y[:, :NB * k], np.zeros((6, NB * k))), "Y above the pose's tile was written"
    ratio = _err_ratio(cov, ref, tol)
    _report(f"pose covariance row0 {row0}", c=ratio)
    assert ratio <= 1


# ---- refusals -------------------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing(gpu):
    api = gpu.api
    m, f = _factor("dense5")
    n = 5 * NB
    B = cc.solve_reference("dense5", "dense")["B"]
    Bb, Xb = _buffers(B, n)

    def refused(call):
        with pytest.raises(api.SlideError) as e:
            call()
        assert e.value.code == -1

    refused(lambda: api.debug_multi_solve(f, Bb, Xb, 0))
    refused(lambda: api.debug_multi_solve(f, Bb, Xb, ALLOC + 1))
    refused(lambda: api.debug_multi_solve(f, Bb, Xb, 4, mode=1, k0=5))
    refused(lambda: api.debug_multi_solve(f, Bb, Xb, 4, mode=1, k0=-1))
    refused(lambda: api.debug_multi_solve(f, Bb, Xb, 4, mode=2))
    refused(lambda: api.debug_multi_solve(dict(f, prof=[4, 4, 3, 4, 4]), Bb, Xb, 4))
    refused(lambda: api.debug_multi_solve(dict(f, prof=[4, 4, 4, 4, 5]), Bb, Xb, 4))
    refused(lambda: api.debug_multi_solve(dict(f, ld=f["ld"] - 1, S=f["S"][:(f["ld"] - 1) * n]), Bb, Xb, 4))
    refused(lambda: api.debug_pose_covariance(f, n - 5))
    refused(lambda: api.debug_pose_covariance(f, -1))
    X, rows, M0, _, _ = cc.gram_case(16, 63, "scattered")
    refused(lambda: api.debug_gram(X, np.r_[rows[:-1], X.shape[1]].astype(np.int32), 63, M0))
    refused(lambda: api.debug_gram(X, None, X.shape[1] + 1, M0))
    refused(lambda: api.debug_gram(X, None, 0, M0))
    _, Xo = api.debug_multi_solve(f, Bb, Xb, 4)
    r = cc.solve_reference("dense5", "dense")
    assert _err_ratio(Xo[:4], r["X"][:4], r["tol_X"]) <= 1
