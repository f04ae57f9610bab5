"""CLIPPER's affinity matrix as CSR (slide_clipper_affinity_csr / _dense_clique_csr / slide_clipper_match): what can be checked without a
device — the symbols, the CSR the reference's golden case must give (numpy restatement on the oracle's matrix), and every refusal of
the host-side check that slide_clipper_dense_clique_csr runs before it touches the device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import slide_slam_amd as s
from oracle import pyoracle as po

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
from test_oracle_pins import MTRUE, _affinity, _model_data  # noqa: E402

NEW = ["slide_clipper_affinity_csr", "slide_clipper_dense_clique_csr", "slide_clipper_match"]


def dense_to_csr(S):
    """(rowptr, col, val) of a dense matrix: rows in order, columns ascending, the stored values bit for bit."""
    S = np.asarray(S, np.float64)
    mask = S != 0
    rowptr = np.concatenate([[0], np.cumsum(mask.sum(axis=1))]).astype(np.int32)
    r, c = np.nonzero(mask)                     # row-major: ascending columns within a row
    return rowptr, c.astype(np.int32), S[r, c]


def test_new_symbols_declared_and_exported():
    txt = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    L = s.lib()
    for f in NEW:
        assert re.search(r"\bint\s+" + f + r"\s*\(", code), f
        assert hasattr(L, f), f
        assert f in s.api.EXPORTS
    assert re.search(r"SLIDE_MS_AFFINITY_CSR\s*=\s*9\b", code) and re.search(r"SLIDE_MS_COUNT\s*=\s*10\b", code)
    assert s.MS_AFFINITY_CSR == 9
    for f in ("clipper_affinity_csr", "clipper_dense_clique_csr", "clipper_match"):
        assert callable(getattr(s, f))


def test_golden_case_as_csr():
    """affinity_test.cpp's 4 x 3 case: the symmetric, diagonal-free CSR of the oracle's upper-filled matrix (what
    M_ = M.sparseView() holds, clipper.cpp:64) is the CSR of the reference's golden MTRUE without its identity."""
    model, data = _model_data()
    m, _, M = _affinity(model, data)
    assert m == 12 and np.array_equal(np.tril(M), np.zeros((12, 12)))
    got = dense_to_csr(M + M.T)
    want = dense_to_csr(MTRUE - np.eye(12))
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)
    rowptr, col, val = got
    assert rowptr[0] == 0 and rowptr[-1] == len(col) == len(val) == int((MTRUE - np.eye(12)).sum())
    for i in range(12):
        c = col[rowptr[i]:rowptr[i + 1]]
        assert np.all(np.diff(c) > 0) and i not in c


def _good():
    """a valid 5-node matrix: edges 0-1, 0-3, 1-3, 2-4"""
    S = np.zeros((5, 5))
    for (i, j, v) in [(0, 1, 0.5), (0, 3, 0.25), (1, 3, 1.0), (2, 4, 0.75)]:
        S[i, j] = S[j, i] = v
    return dense_to_csr(S)


def _refused(rowptr, col, val, row, what):
    with pytest.raises(s.SlideError) as e:
        s.clipper_dense_clique_csr(rowptr, col, val, np.full(len(rowptr) - 1, 0.5))
    msg = str(e.value)
    assert "SLIDE_ERR_INVALID" in msg and f"row {row}:" in msg and what in msg, msg


def test_dense_clique_csr_refuses_a_bad_csr_on_the_host():
    """Every refusal names its row and is reached before the device is: this runs on a machine without one."""
    rowptr, col, val = _good()
    assert rowptr.tolist() == [0, 2, 4, 5, 7, 8] and col.tolist() == [1, 3, 0, 3, 4, 0, 1, 2]
    # rowptr: does not start at 0; decreases; does not end at the arrays' length
    r = rowptr.copy(); r[0] = 1
    _refused(r, col, val, 0, "rowptr[0]")
    r = rowptr.copy(); r[2] = 1                                 # 0 2 1 ...: row 1 ends before it starts
    _refused(r, col, val, 1, "rowptr decreases")
    with pytest.raises(s.SlideError, match="SLIDE_ERR_INVALID.*row 4.*length"):
        s.clipper_dense_clique_csr(rowptr, col[:-1], val[:-1])
    # columns: out of range (both sides); on the diagonal; not ascending; twice
    c = col.copy(); c[4] = 5
    _refused(rowptr, c, val, 2, "outside [0, n)")
    c = col.copy(); c[0] = -1
    _refused(rowptr, c, val, 0, "outside [0, n)")
    c = col.copy(); c[2] = 1                                    # row 1: (1, 1)
    _refused(rowptr, c, val, 1, "diagonal")
    c = col.copy(); c[5], c[6] = 1, 0                           # row 3: 1, 0
    v = val.copy(); v[5], v[6] = val[6], val[5]
    _refused(rowptr, c, v, 3, "ascending")
    c = col.copy(); c[1] = 1                                    # row 0: 1, 1
    _refused(rowptr, c, val, 0, "ascending")
    # symmetry: (0, 3) becomes (0, 2), whose transpose row 2 does not hold; a transpose with another value
    c = col.copy(); c[1] = 2
    _refused(rowptr, c, val, 0, "without its transpose")
    v = val.copy(); v[5] = 0.26                                 # (3, 0) != (0, 3)
    _refused(rowptr, col, v, 0, "another value")
    v = val.copy(); v[3] = np.nan                               # a NaN never equals its transpose
    _refused(rowptr, col, v, 1, "another value")


def test_a_valid_csr_passes_the_host_check():
    """the same matrix unharmed gets past the check: without a device the call then fails as every compute entry point does
    (SLIDE_ERR_HIP, no CPU fallback); an empty problem is answered on the host side of the check alike."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present: the solve runs (tests/test_gpu_affinity_csr.py)")
    rowptr, col, val = _good()
    with pytest.raises(s.SlideError, match="SLIDE_ERR_HIP"):
        s.clipper_dense_clique_csr(rowptr, col, val)
    with pytest.raises(s.SlideError, match="SLIDE_ERR_HIP"):
        s.clipper_match(np.zeros((3, 2)), np.zeros((3, 2)), np.array([[0, 0], [1, 1]], np.int32))
    with pytest.raises(s.SlideError, match="SLIDE_ERR_INVALID.*association 1"):          # checked before the device as well
        s.clipper_match(np.zeros((3, 2)), np.zeros((3, 2)), np.array([[0, 0], [1, 3]], np.int32))
    with pytest.raises(s.SlideError, match="SLIDE_ERR_INVALID.*association 0"):
        s.clipper_affinity_csr(np.zeros((3, 2)), np.zeros((3, 2)), np.array([[-1, 0]], np.int32))
