"""The selected inverse over the exact joint pass's elimination tree (joint_cov_kernels.hip; host side CholBatch::joint_tree /
ensure_joint_sigma in host_marginals.hip), restated in numpy on
synthetic systems laid out like the pass — two robots whose bands fall into segments with a window of poses between them, a separator
of two leaves and a top block, and a lambda block factored as its negative (D = -I) — and checked against np.linalg.inv.  Plus the
C-ABI: the three joint calls are declared in slide_gpu.h and exported by the built library."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
B = 4            # tile edge of the restatement (NB = 64 on the device)


def ldl_blocks(A, sign):
    """Block factor L (lower, non-unit diagonal) with L diag(sign) L^T = A, tile by tile (the pass factors the lambda block's
    negative: sign = -1 there)."""
    n = A.shape[0]
    T = n // B
    L = np.zeros_like(A)
    S = A.copy()
    for k in range(T):
        c = slice(k * B, (k + 1) * B)
        d = sign[k * B]
        Lkk = np.linalg.cholesky(d * S[c, c])
        L[c, c] = Lkk
        below = slice((k + 1) * B, n)
        L[below, c] = d * np.linalg.solve(Lkk, S[below, c].T).T
        S[below, below] -= d * L[below, c] @ L[below, c].T
    return L


def selected_inverse(L, sign, rows_of):
    """Takahashi's recursion from the root down over the tile columns; rows_of(k) = the tile rows I of column k (the stored border rows
    of the node, in ancestor coordinates).  Only Sigma(I, I) of already finished columns is read."""
    n = L.shape[0]
    T = n // B
    Sig = np.full_like(L, np.nan)
    for k in range(T - 1, -1, -1):
        c = slice(k * B, (k + 1) * B)
        Li = np.linalg.inv(L[c, c])
        I = np.concatenate([np.arange(i * B, (i + 1) * B) for i in rows_of(k)]) if rows_of(k) else np.zeros(0, int)
        Z = L[I, c] @ Li
        SII = Sig[np.ix_(I, I)]
        assert not np.isnan(SII).any(), k           # (the row sets are closed under the recursion)
        SIc = -SII @ Z
        Sig[I, c] = SIc
        Sig[c, I] = SIc.T
        Sig[c, c] = sign[k * B] * Li.T @ Li - Z.T @ SIc
    return Sig


def joint_layout(rng, lam_tiles=1):
    """Tiles, in elimination order: robot 0 segment a (3) | robot 0 segment b (2) | robot 1 band (3) | robot 0 window (1) |
    leaf a (2, robot 0's) | leaf b (1, robot 1's) | top (2, both) | lambda (lam_tiles).  Returns A, sign, the structural tile pattern."""
    names = ["s0a"] * 3 + ["s0b"] * 2 + ["b1"] * 3 + ["w0"] + ["la"] * 2 + ["lb"] + ["top"] * 2 + ["lam"] * lam_tiles
    T = len(names)
    couple = {("s0a", "w0"), ("s0b", "w0"), ("s0a", "la"), ("s0b", "la"), ("s0a", "top"), ("s0b", "top"), ("w0", "la"), ("w0", "top"),
              ("b1", "lb"), ("b1", "top"), ("la", "top"), ("lb", "top"), ("s0b", "lam"), ("b1", "lam"), ("w0", "lam")}
    pat = np.zeros((T, T), bool)
    for i in range(T):
        for j in range(T):
            a, b = names[i], names[j]
            if a == b:
                pat[i, j] = abs(i - j) <= 1 or a in ("w0", "top", "la", "lam")      # (bands: tridiagonal in tiles)
            elif (a, b) in couple or (b, a) in couple:
                pat[i, j] = True
    n = T * B
    H = np.zeros((n, n))
    for i in range(T):
        for j in range(i + 1):
            if pat[i, j] and names[i] != "lam" and names[j] != "lam":
                blk = rng.normal(size=(B, B)) * 0.3
                if i == j:
                    blk = blk + blk.T
                H[i * B:(i + 1) * B, j * B:(j + 1) * B] += blk
                if i != j:
                    H[j * B:(j + 1) * B, i * B:(i + 1) * B] += blk.T
    npose = (T - lam_tiles) * B
    H[:npose, :npose] += np.diag(np.abs(H[:npose, :npose]).sum(1) + 1.0)      # (diagonally dominant: SPD with this pattern)
    # the lambda rows: U^T of the relative-pose factors on the poses they touch; [H U; U^T -I]
    nl = lam_tiles * B
    A = H.copy()
    for t in range(T - lam_tiles):
        if pat[T - 1, t]:
            U = rng.normal(size=(nl, B)) * 0.5
            A[npose:, t * B:(t + 1) * B] = U
            A[t * B:(t + 1) * B, npose:] = U.T
    A[npose:, npose:] = -np.eye(nl)
    sign = np.ones(n)
    sign[npose:] = -1.0
    return A, sign, names, npose


def tile_rows(L, k):
    """The tile rows of column k that are non-zero in the factor (what the pass stores: border rows included)."""
    T = L.shape[0] // B
    return [i for i in range(k + 1, T) if np.abs(L[i * B:(i + 1) * B, k * B:(k + 1) * B]).max() > 0]


def test_four_level_recursion_matches_the_dense_inverse():
    rng = np.random.default_rng(3)
    for lam_tiles in (1, 2):
        A, sign, names, npose = joint_layout(rng, lam_tiles)
        L = ldl_blocks(A, sign)
        assert np.allclose(L @ np.diag(sign) @ L.T, A)
        # the leaves never meet: no row of leaf b under a column of leaf a, nor a robot's segment under the other's
        T = len(names)
        for k in range(T):
            for i in tile_rows(L, k):
                assert not (names[k] == "la" and names[i] == "lb")
                assert not (names[k] == "s0a" and names[i] == "s0b")
        Sig = selected_inverse(L, sign, lambda k: tile_rows(L, k))
        ref = np.linalg.inv(A)
        # every entry the recursion formed, the diagonal blocks (the marginals) among them
        done = ~np.isnan(Sig)
        for t in range(T):
            assert done[t * B:(t + 1) * B, t * B:(t + 1) * B].all()
        err = np.abs(np.where(done, Sig - ref, 0.0)).max() / np.abs(ref).max()
        assert err < 1e-12, err
        # the top-left block of inv([H U; U^T -I]) is the true joint marginal (H + U U^T)^-1
        H, U = A[:npose, :npose], A[:npose, npose:]
        P = np.linalg.inv(H + U @ U.T)
        assert np.allclose(Sig[:B, :B], P[:B, :B], rtol=1e-10, atol=1e-12)


def test_a_quasi_definite_lambda_block_needs_its_sign():
    """With D = +I on the lambda block the recursion would invert a different matrix: the sign is what makes it exact."""
    rng = np.random.default_rng(4)
    A, sign, names, npose = joint_layout(rng, 1)
    L = ldl_blocks(A, sign)
    good = selected_inverse(L, sign, lambda k: tile_rows(L, k))
    bad = selected_inverse(L, np.ones_like(sign), lambda k: tile_rows(L, k))
    ref = np.linalg.inv(A)
    assert np.allclose(good[:B, :B], ref[:B, :B], rtol=1e-10)
    assert not np.allclose(bad[:B, :B], ref[:B, :B], rtol=1e-6)


JOINT_CALLS = ["slide_chol_batch_get_pose_covariances", "slide_chol_batch_get_landmark_covariances", "slide_chol_batch_marginal_traces"]


def test_joint_marginal_calls_are_declared_and_exported():
    import slide_slam_amd as s
    hdr = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    L = s.lib()
    for f in JOINT_CALLS:
        assert re.search(r"\bint\s+" + f + r"\s*\(", hdr), f
        assert hasattr(L, f), f
