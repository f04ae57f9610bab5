"""Many loop-closure candidates in one sweep (slide_graph_closure_info_gain_batch / slide_chol_batch_closure_info_gain_batch), without
a GPU: the two entry points are declared and exported, and the block Woodbury identity the sweep rests on, restated in numpy.

One multi-column solve U = H^-1 [J_1^T .. J_K^T] serves every candidate: with U_k its column block, C_k = I + J_k U_k and
M_k = (U_k^T U_k over an index set) — the DIAGONAL blocks only —
    tr(C_k^-1 M_k) = tr(inv(H)) - tr(inv(H + J_k^T J_k))   over that index set,
candidate by candidate.  Taking the stacked J as one candidate (the full C and the full gram, what the single-candidate path would do
with the same columns) answers another question: the drop of all candidates added together."""
import os
import re

import numpy as np

import slide_slam_amd as s

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_entry_points_are_declared_and_exported():
    text = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    L = s.lib()
    for f in ("slide_graph_closure_info_gain_batch", "slide_chol_batch_closure_info_gain_batch"):
        assert re.search(r"\bint\s+" + f + r"\s*\(", text), f
        assert hasattr(L, f) and f in s.api.EXPORTS, f
    assert re.search(r"#define\s+SLIDE_INFO_GAIN_SWEEP_COLS\s+384\b", text)


def test_block_woodbury_per_candidate():
    rng = np.random.default_rng(7)
    n, K = 60, 9
    A = rng.normal(size=(n, n))
    H = A @ A.T + n * np.eye(n)
    S0 = np.linalg.inv(H)
    sets = [np.arange(0, 36), np.arange(36, 60)]                  # ("poses" and "landmarks")
    Js = [rng.normal(size=(6 * int(rng.integers(1, 5)), n)) * (rng.random((1, n)) < 0.3) * 3.0 for _ in range(K)]
    U = np.linalg.solve(H, np.concatenate([J.T for J in Js], axis=1))          # one solve, every candidate's columns side by side
    c0 = np.concatenate([[0], np.cumsum([J.shape[0] for J in Js])])
    status = []
    block = np.zeros((K, len(sets)))
    for k, J in enumerate(Js):
        Uk = U[:, c0[k]:c0[k + 1]]
        C = np.eye(J.shape[0]) + J @ Uk
        C = 0.5 * (C + C.T)
        np.linalg.cholesky(C)                                     # (positive definite: status OK)
        status.append(0)
        S1 = np.linalg.inv(H + J.T @ J)
        for q, idx in enumerate(sets):
            block[k, q] = np.trace(np.linalg.solve(C, Uk[idx].T @ Uk[idx]))
            want = np.trace(S0[np.ix_(idx, idx)]) - np.trace(S1[np.ix_(idx, idx)])
            assert want > 0
            assert abs(block[k, q] - want) <= 1e-10 * abs(want), (k, q, block[k, q], want)
    assert status == [0] * K                                      # every generated candidate is answered
    # the stacked J as ONE candidate: the full C and the full gram give the drop of all candidates together — other numbers
    Jall = np.concatenate(Js)
    Call = np.eye(Jall.shape[0]) + Jall @ U
    Sall = np.linalg.inv(H + Jall.T @ Jall)
    for q, idx in enumerate(sets):
        full = np.trace(np.linalg.solve(Call, U[idx].T @ U[idx]))
        want = np.trace(S0[np.ix_(idx, idx)]) - np.trace(Sall[np.ix_(idx, idx)])
        assert abs(full - want) <= 1e-10 * abs(want)
        assert full < block[:, q].sum() * (1 - 1e-3)              # (information is sub-additive: not the sum of the single drops)
        assert all(abs(full - b) > 1e-3 * abs(b) for b in block[:, q])
