"""The many-right-hand-side solve over the exact joint pass's elimination tree (joint_cov_kernels.hip's k_jms_*; host side
CholBatch::joint_closure_info_gain and its schedule JointTree::solve_plan in host_marginals.hip), restated in numpy on the synthetic layout of tests/test_joint_selected_inverse.py and checked
against np.linalg.solve.  The joint factor is split into the systems the device holds: every robot (its own tiles, then its rows of
separator coordinates, reached through a border map with a padding tile) and the separator.  The schedule is the host's: per node,
forward pushes inside the node and pulls from the nodes below; the robots' separator rows summed into the separator in robot order;
D = -I on the lambda rows; backward pulls from the nodes above and pushes inside the node; the separator's solution gathered back.
Plus the C-ABI: slide_chol_batch_closure_info_gain is declared in slide_gpu.h and exported by the built library."""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from test_joint_selected_inverse import B, joint_layout, ldl_blocks, tile_rows      # noqa: E402

# node -> level: band segments 0, windows 1, a robot's separator rows 2, the separator's leaves 3, top block + lambda 4
LEVEL = {"s0a": 0, "s0b": 0, "b1": 0, "w0": 1, "sep": 2, "la": 3, "lb": 3, "top": 4, "lam": 4}
NODE = {"top": "top", "lam": "top"}          # (the top block and the lambda block are one node)


def split_systems(L, names):
    """The systems of the device: robot r = its own tiles (columns) + its border rows, which hold separator coordinates through a map
    (reversed, with one padding tile: map -1); the separator = the leaf, top and lambda tiles.  Returns per system (tile list of the
    global factor, node names, number of columns, local L) and per robot the map (local border tile -> separator tile or -1)."""
    T = len(names)
    sep_t = [t for t in range(T) if names[t] in ("la", "lb", "top", "lam")]
    own = {0: [t for t in range(T) if names[t] in ("s0a", "s0b", "w0")], 1: [t for t in range(T) if names[t] == "b1"]}
    systems, maps = [], []
    for r in (0, 1):
        touched = sorted({i for k in own[r] for i in tile_rows(L, k) if i in sep_t})
        border = touched[::-1] + [-1]
        tiles = own[r] + border
        Lr = np.zeros((len(tiles) * B, len(own[r]) * B))
        for a, ta in enumerate(tiles):
            for b, tb in enumerate(own[r]):
                if ta >= 0:
                    Lr[a * B:(a + 1) * B, b * B:(b + 1) * B] = L[ta * B:(ta + 1) * B, tb * B:(tb + 1) * B]
        nodes = [names[t] for t in own[r]] + ["sep"] * len(border)
        systems.append((tiles, nodes, len(own[r]), Lr))
        maps.append([sep_t.index(t) if t >= 0 else -1 for t in border])
    Ls = L[np.ix_(np.concatenate([np.arange(t * B, (t + 1) * B) for t in sep_t]),
                  np.concatenate([np.arange(t * B, (t + 1) * B) for t in sep_t]))]
    systems.append((sep_t, [names[t] for t in sep_t], len(sep_t), Ls))
    return systems, maps


def node_of(nm):
    return NODE.get(nm, nm)


def lists(Lr, nodes, ncols):
    """Per tile: forward push rows (same node), backward push columns, forward pull columns (nodes below), backward pull rows."""
    nt = len(nodes)
    fpush, bpush, fpull, bpull = ([[] for _ in range(nt)] for _ in range(4))
    for c in range(ncols):
        for i in tile_rows(Lr, c):
            if node_of(nodes[i]) == node_of(nodes[c]):
                fpush[c].append(i); bpush[i].append(c)
            else:
                fpull[i].append(c); bpull[c].append(i)
    return fpush, bpush, fpull, bpull


def T_(X, k):
    return X[k * B:(k + 1) * B]


def multi_solve(L, names, sign, Bfull, d_sign=True):
    """X = A^-1 Bfull through the tree; Bfull is non-zero on the robots' own rows only (the candidate factors' J^T)."""
    systems, maps = split_systems(L, names)
    nrhs = Bfull.shape[1]
    Xs, info = [], []
    for s, (tiles, nodes, ncols, Lr) in enumerate(systems):
        X = np.zeros((len(tiles) * B, nrhs))
        for a, t in enumerate(tiles[:ncols] if s < 2 else []):      # (the separator's right-hand side comes from the sum)
            X[a * B:(a + 1) * B] = Bfull[t * B:(t + 1) * B]
        Xs.append(X)
        info.append(lists(Lr, nodes, ncols))
    Lt = lambda s, i, k: systems[s][3][i * B:(i + 1) * B, k * B:(k + 1) * B]       # noqa: E731
    Dneg = [[d_sign and sign[t * B] < 0 for t in systems[s][0]] for s in range(3)]

    def levels_cols(s, lev):
        tiles, nodes, ncols, _ = systems[s]
        groups = {}
        for k in range(ncols):
            if LEVEL[nodes[k]] == lev:
                groups.setdefault(node_of(nodes[k]), []).append(k)
        return list(groups.values())

    def push(s, lev, bwd):
        groups = levels_cols(s, lev)
        for st in range(max((len(g) for g in groups), default=0)):
            for g in groups:                                     # (side by side on the device: no shared target)
                if st >= len(g):
                    continue
                k = g[-1 - st] if bwd else g[st]
                X = Xs[s]
                Lkk = Lt(s, k, k)
                if bwd:
                    x = np.linalg.solve(Lkk.T, T_(X, k))
                    for j in info[s][1][k]:
                        T_(X, j)[:] -= Lt(s, k, j).T @ x
                else:
                    x = np.linalg.solve(Lkk, T_(X, k))
                    for i in info[s][0][k]:
                        T_(X, i)[:] -= Lt(s, i, k) @ x
                T_(X, k)[:] = x

    def pull(s, lev, bwd):
        tiles, nodes, ncols, _ = systems[s]
        X = Xs[s]
        for k in range(len(tiles)):
            if LEVEL[nodes[k]] != lev or (bwd and k >= ncols):
                continue
            if bwd:
                t = -T_(X, k) if Dneg[s][k] else T_(X, k).copy()
                for i in info[s][3][k]:
                    t -= Lt(s, i, k).T @ T_(X, i)
            else:
                t = T_(X, k).copy()
                for j in info[s][2][k]:
                    t -= Lt(s, k, j) @ T_(X, j)
            T_(X, k)[:] = t

    S = 2
    for r in (0, 1):
        push(r, 0, False)
        pull(r, 1, False); push(r, 1, False)
        pull(r, 2, False)
    # the separator's right-hand side: the robots' separator rows, robot by robot through the inverse of the maps
    Xs[S][:] = 0.0
    for r in (0, 1):
        ncols = systems[r][2]
        for o, st in enumerate(maps[r]):
            if st >= 0:
                T_(Xs[S], st)[:] += T_(Xs[r], ncols + o)
    push(S, 3, False)
    pull(S, 4, False); push(S, 4, False)
    pull(S, 4, True); push(S, 4, True)
    pull(S, 3, True); push(S, 3, True)
    for r in (0, 1):                                           # the gather (padding: 0)
        ncols = systems[r][2]
        for o, st in enumerate(maps[r]):
            T_(Xs[r], ncols + o)[:] = T_(Xs[S], st) if st >= 0 else 0.0
        pull(r, 1, True); push(r, 1, True)
        pull(r, 0, True); push(r, 0, True)
    out = np.zeros_like(Bfull)
    for s, (tiles, nodes, ncols, _) in enumerate(systems):
        for a, t in enumerate(tiles[:ncols]):
            out[t * B:(t + 1) * B] = T_(Xs[s], a)
    return out, systems, maps


def rhs(rng, names, nrhs):
    Bf = np.zeros((len(names) * B, nrhs))
    for t, nm in enumerate(names):
        if nm in ("s0a", "s0b", "b1", "w0"):
            Bf[t * B:(t + 1) * B] = rng.normal(size=(B, nrhs))
    return Bf


def test_tree_layout_has_every_edge():
    """The layout exercises what the schedule has to get right: border rows of both segments in the window, a padding tile in each
    border map, leaves that never meet, a lambda block, and separator tiles reached from both robots (the slot-ordered sum)."""
    rng = np.random.default_rng(5)
    A, sign, names, npose = joint_layout(rng, 1)
    L = ldl_blocks(A, sign)
    systems, maps = split_systems(L, names)
    assert all(-1 in m for m in maps)
    both = set(m for m in maps[0] if m >= 0) & set(m for m in maps[1] if m >= 0)
    assert both, maps
    tiles0, nodes0, ncols0, L0 = systems[0]
    fpush, bpush, fpull, bpull = lists(L0, nodes0, ncols0)
    w = nodes0.index("w0")
    assert {nodes0[j] for j in fpull[w]} == {"s0a", "s0b"}
    assert any(nodes0[i] == "sep" for i in bpull[w])


def test_solve_matches_numpy():
    rng = np.random.default_rng(6)
    for lam_tiles in (1, 2):
        A, sign, names, npose = joint_layout(rng, lam_tiles)
        L = ldl_blocks(A, sign)
        for nrhs in (1, 7, 384):
            Bf = rhs(rng, names, nrhs)
            got, _, _ = multi_solve(L, names, sign, Bf)
            want = np.linalg.solve(A, Bf)
            err = np.abs(got - want).max() / np.abs(want).max()
            assert err < 1e-11, (lam_tiles, nrhs, err)
        # the primal rows are (H + U U^T)^-1 B: the joint marginal model the gain's Woodbury step uses
        H, U = A[:npose, :npose], A[:npose, npose:]
        Bf = rhs(rng, names, 3)
        got, _, _ = multi_solve(L, names, sign, Bf)
        assert np.allclose(got[:npose], np.linalg.solve(H + U @ U.T, Bf[:npose]), rtol=1e-9, atol=1e-12)


def test_lambda_rows_need_their_sign():
    """Without the D step (D = +I on the lambda block) the solve is finite but wrong."""
    rng = np.random.default_rng(7)
    A, sign, names, npose = joint_layout(rng, 1)
    L = ldl_blocks(A, sign)
    Bf = rhs(rng, names, 7)
    want = np.linalg.solve(A, Bf)
    good, _, _ = multi_solve(L, names, sign, Bf)
    bad, _, _ = multi_solve(L, names, sign, Bf, d_sign=False)
    assert np.isfinite(bad).all()
    assert np.allclose(good, want, rtol=1e-9, atol=1e-12)
    assert not np.allclose(bad[:npose], want[:npose], rtol=1e-6)


def test_joint_closure_info_gain_is_declared_and_exported():
    import slide_slam_amd as s
    hdr = open(os.path.join(ROOT, "include", "slide_gpu.h")).read()
    f = "slide_chol_batch_closure_info_gain"
    assert re.search(r"\bint\s+" + f + r"\s*\(", hdr), f
    assert hasattr(s.lib(), f), f
